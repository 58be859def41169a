"""GPU tests (pytest -m gpu) of csmp_ard_weights and csmp_ista_reweighted against the numpy Float64 twin of tests/reweight_twin.py.
Weights: |w² − w_twin²| ≤ the bound of reweight_twin.ard_tolerance, per atom (derived there, not tuned; the observed error is printed
beside it).  Solutions: ista_twin.compare at RTOL = 1e-6, the suite's contract."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ista_twin as tw  # noqa: E402
import reweight_twin as rt  # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHT_PARAMS = [(name, it, ones) for name in rt.WEIGHT_CASES for it in (1, 8) for ones in (True, False)]
SOLVE_PARAMS = [(shape, scheme, accel) for shape in rt.SOLVE_SHAPES for scheme in ("candes", "ard") for accel in (False, True)]


def _wid(p):
    return f"{p[0]}-iter{p[1]}-{'ones' if p[2] else 'random'}"


def _sid(p):
    return f"{p[0]}-{p[1]}-{'fista' if p[2] else 'ista'}"


# ------------------------------------------------------------------------------------------ ard_weights
@pytest.mark.parametrize("case", WEIGHT_PARAMS, ids=_wid)
def test_ard_weights_match_the_twin(cs, case):
    """32 x 48 (M below one 64-row block), 256 x 1024 Float32, 261 x 1000 in both types with 150 atoms planted (two direction blocks,
    the second of 22; a last row block of 5 rows; N no multiple of 128), 1000 x 300 with 130 (128 | 2), k = 0, k = 1, a support with
    atoms 0 and N - 1; iter 1 and 8; from ones and from random weights in [0.5, 2]"""
    name, it, ones = case
    A, x, w_in = rt.weight_case(name)
    wt, bound, kappa = rt.weight_twin(name, it, ones)
    D = cs.Dictionary(A)
    try:
        w = D.ctx.ard_weights(x, None if ones else w_in, rt.EPS, it)
    finally:
        D.close()
    rt.compare_weights(w, wt, bound, f"{_wid(case)} (k = {np.count_nonzero(x)}, kappa = {kappa:.2e})")


def test_api_weights(cs):
    A, x, w_in = rt.weight_case("256x1024_f32_k16")
    wt, bound, _ = rt.weight_twin("256x1024_f32_k16", 8, False)
    keep = w_in.copy()
    w = cs.ard_weights(A, cs.SparseVector(len(x), np.flatnonzero(x), x[np.flatnonzero(x)]), w_in)
    assert np.array_equal(w_in, keep)  # (the weights passed in are not changed)
    rt.compare_weights(w, wt, bound, "api")
    assert np.array_equal(cs.candes_weights(x, 1e-2), rt.candes_weights(x, 1e-2))
    for bad in (lambda: cs.candes_weights(x, 0.0), lambda: cs.ard_weights(A, x, w_in, eps=-1.0), lambda: cs.ard_weights(A, x, w_in, iter=0),
                lambda: cs.ard_weights(A, x, np.where(np.arange(len(x)) == 5, 0.0, w_in)), lambda: cs.ard_weights(A, x[:-1])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ refusals
def _raw_ard(L, ctx, x, w, eps, it):
    out = np.zeros(max(len(x), 1))
    return L.lib().csmp_ard_weights(ctx._h, L.ptr(x), L.ptr(w), C.c_double(eps), L.i64(it), L.ptr(out), L.HOST)


def _raw_solve(L, ctx, b, lam=rt.LAMBDA, scheme=0, eps=rt.EPS, ard_iter=8, outer=4, md=0.0, maxiter=8, stepsize=1e-2, accel=0):
    x = np.zeros(max(ctx.N, 1))
    done, rn = L.i64(0), C.c_double(0)
    return L.lib().csmp_ista_reweighted(ctx._h, L.ptr(b), L.dtype_code(b.dtype), C.c_double(lam), scheme, C.c_double(eps), L.i64(ard_iter),
                                        L.i64(outer), C.c_double(md), L.i64(maxiter), C.c_double(stepsize), accel, L.ptr(x), L.HOST, None,
                                        C.byref(done), C.byref(rn))


def test_refusals(cs):
    L = cs._lib
    A, _, b, alpha, _ = tw.case_data("32x48_f64")
    M, N = A.shape
    _, x3, _ = rt.weight_case("32x48_f64_k3")
    ones = np.ones(N)
    want_w = rt.ard_support(A, x3, None, rt.EPS, 8)
    bound, _ = rt.ard_tolerance(A, x3, None, rt.EPS, 8)

    ctx = cs.Context(0)  # no dictionary set
    assert _raw_ard(L, ctx, x3, ones, rt.EPS, 8) == L.ESTATE
    assert _raw_solve(L, ctx, b) == L.ESTATE
    ctx.close()
    D = cs.Dictionary(A, streamed=True)  # a host-streamed dictionary
    assert _raw_ard(L, D.ctx, x3, ones, rt.EPS, 8) == L.ESTATE
    assert "streamed" in L.lib().csmp_last_error(D.ctx._h).decode()
    assert _raw_solve(L, D.ctx, b) == L.ESTATE
    D.close()

    D = cs.Dictionary(A)
    ctx = D.ctx

    def still_solves():
        rt.compare_weights(ctx.ard_weights(x3, None, rt.EPS, 8), want_w, bound, "after a refusal")
        x, _, done = ctx.ista_reweighted(b, rt.LAMBDA, "ard", outer_maxiter=2, maxiter=64, stepsize=alpha, min_decrease=0.0)
        assert done == 2
        tw.compare(x, rt.reweighted(A, b, rt.LAMBDA, rt.ARD, rt.EPS, 8, 2, 0.0, 64, alpha)[0])

    for j in (0, 7, N - 1):  # a zero weight, wherever it sits (the reference: "weights cannot be zero")
        w = ones.copy()
        w[j] = 0.0
        assert _raw_ard(L, ctx, x3, w, rt.EPS, 8) == L.EINVAL, j
        assert "zero" in L.lib().csmp_last_error(ctx._h).decode()
    still_solves()
    for bad in (-1.0, float("nan"), float("inf")):
        w = ones.copy()
        w[3] = bad
        assert _raw_ard(L, ctx, x3, w, rt.EPS, 8) == L.EINVAL, bad
    for bad in (0.0, -1e-2, float("nan"), float("inf")):
        assert _raw_ard(L, ctx, x3, ones, bad, 8) == L.EINVAL, bad
        assert _raw_solve(L, ctx, b, eps=bad) == L.EINVAL, bad
        assert _raw_solve(L, ctx, b, eps=bad, scheme=1) == L.EINVAL, bad
    still_solves()
    x33 = np.zeros(N)
    x33[:33] = 1.0  # 33 non-zeros at M = 32
    assert _raw_ard(L, ctx, x33, ones, rt.EPS, 8) == L.ERANGE
    still_solves()
    x32 = x33.copy()
    x32[32] = 0.0  # (32 of them are taken)
    assert _raw_ard(L, ctx, x32, ones, rt.EPS, 1) == L.OK
    assert _raw_ard(L, ctx, x3, ones, rt.EPS, 0) == L.EINVAL  # iter < 1
    for scheme in (0, 1):
        assert _raw_solve(L, ctx, b, scheme=scheme, ard_iter=0) == L.EINVAL
        assert _raw_solve(L, ctx, b, scheme=scheme, outer=0) == L.EINVAL
    assert _raw_solve(L, ctx, b, scheme=2) == L.EINVAL
    assert _raw_solve(L, ctx, b, md=-1.0) == L.EINVAL
    assert _raw_solve(L, ctx, b, md=float("nan")) == L.EINVAL
    assert _raw_solve(L, ctx, b, lam=-1.0) == L.EINVAL
    assert _raw_solve(L, ctx, b, maxiter=-1) == L.EINVAL
    assert _raw_solve(L, ctx, b, stepsize=0.0) == L.EINVAL
    assert _raw_solve(L, ctx, b, accel=2) == L.EINVAL
    still_solves()
    D.close()


# ------------------------------------------------------------------------------------------ the reweighted solves
def _solve(ctx, shape, scheme, accel, **kw):
    A, _, b, alpha, inner = tw.case_data(shape)
    kw.setdefault("outer_maxiter", rt.OUTER)
    kw.setdefault("min_decrease", 0.0)
    return ctx.ista_reweighted(b, rt.LAMBDA, scheme, eps=rt.EPS, ard_iter=8, maxiter=inner, stepsize=alpha, accel=accel, **kw)


def _weight_bound(A, scheme, twin):
    """the tolerance of the returned weights, on w²: ARD -- reweight_twin.ard_tolerance for the x and w the last reweighting started
    from; Candès -- w = 1 / (|x| + ε) with |Δx_j| ≤ RTOL · max|x_twin| (the solution's contract) gives |Δw_j| ≤ w_j² · that + 4u w_j,
    and |Δw_j²| ≤ 2 w_j |Δw_j| (1 + 1e-6)"""
    xt, wt, _, _, (x_last, w_last) = twin
    if scheme == "ard":
        return rt.ard_tolerance(A, x_last, w_last, rt.EPS, 8)[0]
    dw = wt ** 2 * tw.band(x_last) + 4 * 2.0 ** -53 * wt
    return 2 * wt * dw * (1 + 1e-6)


@pytest.mark.parametrize("case", SOLVE_PARAMS, ids=_sid)
def test_reweighted_solves_match_the_twin(cs, case):
    """λ = 2e-2, ε = 1e-2, min_decrease = 0: exactly 8 solves of 1024 iterations; ista and fista (λ = 2e-2 only: DESIGN.md §10)"""
    shape, scheme, accel = case
    A, x0, b, _, _ = tw.case_data(shape)
    twin = rt.solve_twin(shape, scheme, accel)
    D = cs.Dictionary(A)
    try:
        x, rn, done, w = _solve(D.ctx, shape, scheme, accel, return_weights=True)
    finally:
        D.close()
    assert done == rt.OUTER == twin[2]
    res = float(np.linalg.norm(b.astype(np.float64) - A.astype(np.float64) @ x))
    print(f"{_sid(case)}: resnorm {rn:.12e}  numpy on the returned x {res:.12e}  nnz {np.count_nonzero(x)}")
    assert abs(rn - res) <= 1e-9 * max(1.0, res)
    tw.compare(x, twin[0])
    assert np.array_equal(np.flatnonzero(x), np.flatnonzero(x0))  # (the reference's property, test/basispursuit.jl:18-22)
    rt.compare_weights(w, twin[1], _weight_bound(A, scheme, twin), "the returned weights")


@pytest.mark.parametrize("scheme", ["candes", "ard"])
def test_early_exit(cs, scheme):
    shape = "32x48_f64"
    A, _, _, _, _ = tw.case_data(shape)
    h = rt.solve_twin(shape, scheme, False)[3]
    print("step norms of the twin:", " ".join(f"{v:.2e}" for v in h))
    assert h[2] / h[3] >= 25  # (a condition on the instance: the threshold sits well inside the gap)
    md = float(np.sqrt(h[2] * h[3]))
    twin = rt.solve_twin(shape, scheme, False, md)
    assert twin[2] == 5
    D = cs.Dictionary(A)
    x, _, done = _solve(D.ctx, shape, scheme, False, min_decrease=md)
    D.close()
    assert done == 5  # the first solve and four re-solves
    tw.compare(x, twin[0])


@pytest.mark.parametrize("accel", [False, True])
def test_outer_maxiter_1_is_the_plain_solve(cs, accel):
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    D = cs.Dictionary(A)
    want = D.ctx.ista(b, rt.LAMBDA, maxiter=300, stepsize=alpha, accel=accel)
    for scheme in ("candes", "ard"):
        x, rn, done, w = D.ctx.ista_reweighted(b, rt.LAMBDA, scheme, outer_maxiter=1, maxiter=300, stepsize=alpha, accel=accel, return_weights=True)
        assert done == 1 and np.array_equal(x, want[0]) and rn == want[1] and np.array_equal(w, np.ones(len(x)))
    D.close()


def test_two_runs_give_the_same_bits(cs):
    A, x, w_in = rt.weight_case("261x1000_f32_k150")
    D = cs.Dictionary(A)
    w1 = D.ctx.ard_weights(x, w_in, rt.EPS, 8)
    small = D.ctx.ard_weights(np.where(np.arange(len(x)) < 100, x, 0.0), w_in, rt.EPS, 8)  # (another support size in between)
    w2 = D.ctx.ard_weights(x, w_in, rt.EPS, 8)
    D.close()
    D = cs.Dictionary(A)  # (and from a fresh context)
    w3 = D.ctx.ard_weights(x, w_in, rt.EPS, 8)
    D.close()
    assert np.array_equal(w1, w2) and np.array_equal(w1, w3) and not np.array_equal(w1, small)
    shape = "256x1024_f32"
    A = tw.case_data(shape)[0]
    for scheme in ("candes", "ard"):
        for accel in (False, True):
            D = cs.Dictionary(A)
            r1 = _solve(D.ctx, shape, scheme, accel, outer_maxiter=4, return_weights=True)
            r2 = _solve(D.ctx, shape, scheme, accel, outer_maxiter=4, return_weights=True)
            D.close()
            D = cs.Dictionary(A)
            r3 = _solve(D.ctx, shape, scheme, accel, outer_maxiter=4, return_weights=True)
            D.close()
            for r in (r2, r3):
                assert np.array_equal(r1[0], r[0]) and r1[1] == r[1] and r1[2] == r[2] == 4 and np.array_equal(r1[3], r[3]), (scheme, accel)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_pointers(cs, dtype):
    import torch
    shape = "256x1024_f32"
    A, _, b, alpha, inner = tw.case_data(shape)
    N = A.shape[1]
    D = cs.Dictionary(A)
    for scheme in ("candes", "ard"):
        want = D.ctx.ista_reweighted(b.astype(dtype), rt.LAMBDA, scheme, outer_maxiter=3, min_decrease=0.0, maxiter=inner, stepsize=alpha, accel=True,
                                     return_weights=True)
        bt = torch.from_numpy(b.astype(dtype)).cuda()
        xt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        wt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        rn, done = D.ctx.ista_reweighted_device(bt, rt.LAMBDA, scheme, xt, wt, outer_maxiter=3, min_decrease=0.0, maxiter=inner, stepsize=alpha, accel=True)
        assert np.array_equal(xt.cpu().numpy(), want[0]) and rn == want[1] and done == want[2] == 3 and np.array_equal(wt.cpu().numpy(), want[3])
        rn2, _ = D.ctx.ista_reweighted_device(bt, rt.LAMBDA, scheme, xt, None, outer_maxiter=3, min_decrease=0.0, maxiter=inner, stepsize=alpha, accel=True)
        assert rn2 == rn and np.array_equal(xt.cpu().numpy(), want[0])
    _, x, w_in = rt.weight_case("256x1024_f32_k16")
    want_w = D.ctx.ard_weights(x, w_in, rt.EPS, 8)
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w_in).cuda()
    out = torch.zeros(N, dtype=torch.float64, device="cuda")
    D.ctx.ard_weights_device(xd, wd, out, rt.EPS, 8)
    assert np.array_equal(out.cpu().numpy(), want_w) and np.array_equal(wd.cpu().numpy(), w_in)
    D.ctx.ard_weights_device(xd, wd, wd, rt.EPS, 8)  # in place
    assert np.array_equal(wd.cpu().numpy(), want_w)
    D.close()


# ------------------------------------------------------------------------------------------ allocations, other solvers
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_ista.py's pattern: every allocation of csmp_ard_weights and of csmp_ista_reweighted fails in turn with CSMP_ENOMEM,
    the same context then returns the clean context's bits, and the library holds what it held before."""
    L = cs._lib
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    _, x, w_in = rt.weight_case("256x1024_f32_k16")
    gc.collect()
    base = L.live_resources()

    def weights(ctx):
        return (ctx.ard_weights(x, w_in, rt.EPS, 2),)

    def solve(ctx):
        return ctx.ista_reweighted(b, rt.LAMBDA, "ard", ard_iter=2, outer_maxiter=2, min_decrease=0.0, maxiter=16, stepsize=alpha, return_weights=True)

    for call, least in ((weights, 19), (solve, 19)):  # (the 8 dictionary-sized and the 11 support-sized buffers; the solve's come after ista's)
        clean = cs.Dictionary(A)
        want = call(clean.ctx)
        clean.close()
        n, seen_ok, failed = 0, 0, 0
        while seen_ok < 2 and n < 200:
            n += 1
            d = cs.Dictionary(A)
            d.ctx.tune("fail_alloc", n)
            try:
                got = call(d.ctx)
                assert all(np.array_equal(u, v) for u, v in zip(got, want)), n
                seen_ok += 1
            except cs.CsmpError as e:
                seen_ok = 0
                failed += 1
                assert e.code == L.ENOMEM, (n, e.code, str(e))
            d.ctx.tune("fail_alloc", 0)
            got = call(d.ctx)
            assert all(np.array_equal(u, v) for u, v in zip(got, want)), (n, "after the failed call")
            d.close()
        print(f"{call.__name__}: {failed} allocations failed in turn")
        assert n < 200 and failed >= least
        gc.collect()
        assert L.live_resources() == base


def test_other_solvers_are_not_disturbed(cs):
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    _, x, w_in = rt.weight_case("256x1024_f32_k16")
    eps = float(np.finfo(np.float32).eps)
    D = cs.Dictionary(A)
    before = D.ctx.omp(b, 16, eps)
    mp_before = D.ctx.mp(b, 24)
    x1 = D.ctx.ista(b, rt.LAMBDA, maxiter=50, stepsize=alpha)
    w1 = D.ctx.ard_weights(x, w_in, rt.EPS, 8)
    r1 = D.ctx.ista_reweighted(b, rt.LAMBDA, "ard", outer_maxiter=3, maxiter=64, stepsize=alpha, min_decrease=0.0)
    after = D.ctx.omp(b, 16, eps)
    x2 = D.ctx.ista(b, rt.LAMBDA, maxiter=50, stepsize=alpha)
    r2 = D.ctx.ista_reweighted(b, rt.LAMBDA, "candes", outer_maxiter=3, maxiter=64, stepsize=alpha, min_decrease=0.0)
    w2 = D.ctx.ard_weights(x, w_in, rt.EPS, 8)
    mp_after = D.ctx.mp(b, 24)
    assert all(np.array_equal(u, v) for u, v in zip(mp_before, mp_after))
    D.close()
    assert all(np.array_equal(u, v) for u, v in zip(before, after))
    assert np.array_equal(x1[0], x2[0]) and x1[1] == x2[1] and np.array_equal(w1, w2) and r1[0].any() and r2[0].any()


def test_api_returns_sparse_vectors(cs):
    A, x0, b, alpha, inner = tw.case_data("256x1024_f32")
    for fn, scheme in ((cs.ista_candes, "candes"), (cs.ista_ard, "ard")):
        x, w = fn(A, b, rt.LAMBDA, rt.EPS, maxiter=rt.OUTER, min_decrease=0.0, inner_maxiter=inner, stepsize=alpha, return_weights=True)
        assert isinstance(x, cs.SparseVector) and x.n == A.shape[1] and np.all(x.nzval != 0) and np.all(np.diff(x.nzind) > 0)
        assert np.array_equal(x.nzind, np.flatnonzero(x0)) and w.shape == (A.shape[1],)
        tw.compare(x.to_dense(), rt.solve_twin("256x1024_f32", scheme, False)[0])
        D = cs.Dictionary(A)
        xf = fn(D, b, rt.LAMBDA, maxiter=2, inner_maxiter=64, stepsize=alpha, accel=True)
        D.close()
        assert isinstance(xf, cs.SparseVector)
        with pytest.raises(ValueError):
            fn(A, b, rt.LAMBDA, maxiter=0)
        with pytest.raises(ValueError):
            fn(A, b, rt.LAMBDA, 0.0)
