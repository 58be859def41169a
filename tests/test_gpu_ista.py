"""GPU tests (pytest -m gpu) of csmp_ista: ista (src/basispursuit.jl:164-183) and FISTA against the numpy Float64 twin of
tests/ista_twin.py, at the suite's tolerance: |x − x_twin| ≤ 1e-6 · max|x_twin| for every coordinate, the same support outside the
band |x_j| ≤ atol on either side, at most N/100 coordinates in the band (tests/test_ista_static.py: none of the twin's own)."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ista_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu

ISTA_CASES = [c for c in tw.parity_cases() if c[0] == "ista"]
FISTA_CASES = [c for c in tw.parity_cases() if c[0] == "fista"]


def _run(cs, case):
    A, b, w, x0, maxiter, alpha = tw.case_args(case)
    D = cs.Dictionary(A)
    try:
        i0, v0 = (None, None) if x0 is None else x0
        x, rn = D.ctx.ista(b, w, i0, v0, maxiter=maxiter, stepsize=alpha, accel=case[0] == "fista")
    finally:
        D.close()
    res = float(np.linalg.norm(b.astype(np.float64) - A.astype(np.float64) @ x))
    print(f"{tw.case_id(case)}: resnorm {rn:.12e}  numpy on the returned x {res:.12e}")
    assert abs(rn - res) <= 1e-9 * max(1.0, res)
    return x


@pytest.mark.parametrize("case", ISTA_CASES, ids=tw.case_id)
def test_ista_matches_the_twin(cs, case):
    """shapes: the reference's 32 x 48, 256 x 1024 and 512 x 4096 Float32, short columns, a ragged Float64 one, a residual longer than
    the LDS; λ = 1e-3 (most atoms alive), 2e-2 and 0.2 (few); a weight vector with zero weights; a warm start"""
    tw.compare(_run(cs, case), tw.case_twin(case))


@pytest.mark.parametrize("case", FISTA_CASES, ids=tw.case_id)
def test_fista_matches_the_twin(cs, case):
    """λ = 2e-2 and 0.2 only.  At λ = 1e-3 the FISTA iteration is not defined to this tolerance between two CPU runs of the same
    formulas (Float64 against 80-bit long double against permuted rows, 1024 iterations: up to 1.0e-5 · max|x| and one or two support
    flips at 512 x 4096): a comparison there would measure the summation order, not the library."""
    tw.compare(_run(cs, case), tw.case_twin(case))


def test_fista_objective_is_ahead_after_200(cs):
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    D = cs.Dictionary(A)
    xf, _ = D.ctx.ista(b, 2e-2, maxiter=200, stepsize=alpha, accel=True)
    xi, _ = D.ctx.ista(b, 2e-2, maxiter=200, stepsize=alpha, accel=False)
    D.close()
    ff, fi = tw.objective(A, b, 2e-2, xf), tw.objective(A, b, 2e-2, xi)
    print(f"objective after 200: fista {ff:.12e}  ista {fi:.12e}")
    assert ff <= fi


def test_api_returns_sparse_vectors(cs):
    case = ("ista", "256x1024_f32", 0.2)
    A, b, w, _, maxiter, alpha = tw.case_args(case)
    xt = tw.case_twin(case)
    x = cs.ista(A, b, w, maxiter=maxiter, stepsize=alpha)
    assert isinstance(x, cs.SparseVector) and x.n == A.shape[1] and np.all(x.nzval != 0) and np.all(np.diff(x.nzind) > 0)
    tw.compare(x.to_dense(), xt)
    D = cs.Dictionary(A)
    warm = cs.SparseVector(A.shape[1], [5, 900, 17], [0.3, -0.2, 0.1])
    keep = warm.copy()
    xf = cs.fista(D, b, np.full(A.shape[1], 0.2), warm, maxiter=64, stepsize=alpha)
    D.close()
    assert np.array_equal(warm.nzind, keep.nzind) and np.array_equal(warm.nzval, keep.nzval)  # (the warm start is not changed)
    tw.compare(xf.to_dense(), tw.fista(A, b, 0.2, (keep.nzind, keep.nzval), 64, alpha))


# ------------------------------------------------------------------------------------------ edge cases
def test_maxiter_0_and_1(cs):
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    N = A.shape[1]
    D = cs.Dictionary(A)
    x, rn = D.ctx.ista(b, 2e-2, maxiter=0, stepsize=alpha)
    assert not x.any() and abs(rn - np.linalg.norm(b.astype(np.float64))) <= 1e-12 * rn
    idx, val = np.array([700, 3, 41]), np.array([0.5, -1.25, 2.0])
    for accel in (False, True):
        x, rn = D.ctx.ista(b, 2e-2, idx, val, maxiter=0, stepsize=alpha, accel=accel)
        want = tw.dense((idx, val), N)
        assert np.array_equal(x, want)  # maxiter = 0 returns the warm start
        res = np.linalg.norm(b.astype(np.float64) - A.astype(np.float64) @ want)
        assert abs(rn - res) <= 1e-12 * res
        x1, _ = D.ctx.ista(b, 2e-2, maxiter=1, stepsize=alpha, accel=accel)
        tw.compare(x1, tw.ista(A, b, 2e-2, None, 1, alpha))  # (the first FISTA step is the ISTA step: t₁ = 1)
        x1w, _ = D.ctx.ista(b, 2e-2, idx, val, maxiter=1, stepsize=alpha, accel=accel)
        tw.compare(x1w, tw.ista(A, b, 2e-2, (idx, val), 1, alpha))
    D.close()


def test_zero_signal_and_large_lambda_give_exact_zeros(cs):
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    D = cs.Dictionary(A)
    for accel in (False, True):
        x, rn = D.ctx.ista(np.zeros_like(b), 2e-2, maxiter=16, stepsize=alpha, accel=accel)
        assert not x.any() and rn == 0.0
        lam = 2.5 * float(np.max(np.abs(A.astype(np.float64).T @ b.astype(np.float64))))  # |2α c_j| < λα for every atom: x stays 0
        x, rn = D.ctx.ista(b, lam, maxiter=16, stepsize=alpha, accel=accel)
        assert not x.any() and abs(rn - np.linalg.norm(b.astype(np.float64))) <= 1e-12 * rn
    D.close()
    assert cs.ista(A, np.zeros_like(b), 2e-2, maxiter=4, stepsize=alpha).nnz == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_pointers(cs, dtype):
    import torch
    case = ("fista", "256x1024_f32", 2e-2)
    A, b, w, _, maxiter, alpha = tw.case_args(case)
    D = cs.Dictionary(A)
    want, rn_host = D.ctx.ista(b.astype(dtype), w, maxiter=maxiter, stepsize=alpha, accel=True)
    bt = torch.from_numpy(b.astype(dtype)).cuda()
    xt = torch.full((A.shape[1],), 7.0, dtype=torch.float64, device="cuda")
    rn = D.ctx.ista_device(bt, w, xt, maxiter=maxiter, stepsize=alpha, accel=True)
    got = xt.cpu().numpy()
    D.close()
    assert np.array_equal(got, want) and rn == rn_host
    tw.compare(got, tw.case_twin(case))


# ------------------------------------------------------------------------------------------ the benchmark shape
def _bench_problem(torch):
    g = torch.Generator(device="cuda").manual_seed(11)
    M, N, k = 4096, 65536, 256
    A = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)  # rows are atoms
    A /= A.norm(dim=1, keepdim=True)
    A = A.to(torch.float32).contiguous()
    S = torch.randperm(N, generator=g, device="cuda")[:k]
    xs = torch.zeros(N, dtype=torch.float64, device="cuda")
    xs[S] = torch.where(torch.rand(k, generator=g, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
    A64 = A.to(torch.float64)
    b = (xs @ A64 + 5e-3 * torch.randn(M, generator=g, device="cuda", dtype=torch.float64)).to(torch.float32)
    v = torch.randn(N, generator=g, device="cuda", dtype=torch.float64)
    for _ in range(40):  # ‖A‖₂² by power iteration on A Aᵀ
        v = A64 @ (v @ A64)
        s = v.norm()
        v /= s
    return A, A64, b, 0.45 / float(s)


def _torch_iteration(torch, A64, b, lam, maxiter, alpha, accel):
    """the same iteration in torch Float64 on the card, on the promoted dictionary (A64: rows are atoms)"""
    b = b.to(torch.float64)
    x = torch.zeros(A64.shape[0], dtype=torch.float64, device="cuda")
    y, t = x.clone(), 1.0
    for _ in range(maxiter):
        g = A64 @ (b - y @ A64)
        u = y + 2 * alpha * g
        xn = torch.sign(u) * torch.clamp(u.abs() - lam * alpha, min=0.0)
        tn = (1.0 + (1.0 + 4.0 * t * t) ** 0.5) / 2.0
        y = xn + ((t - 1.0) / tn) * (xn - x) if accel else xn
        x, t = xn, tn
    return (x + 0.0).cpu().numpy()


def test_benchmark_shape_against_torch_float64(cs):
    """4096 x 65536 Float32, 32 iterations, λ = 1.6 (iterates near the planted 256 non-zeros) and λ = 1e-3 (more than N/2 alive),
    against the same iteration in torch Float64 on the card; and the same bits from a second run."""
    import torch
    A, A64, b, alpha = _bench_problem(torch)
    D = cs.Dictionary(A)
    N = A.shape[0]
    for lam, dense in ((1.6, False), (1e-3, True)):
        for accel in (False, True):
            xt = torch.zeros(N, dtype=torch.float64, device="cuda")
            D.ctx.ista_device(b, lam, xt, maxiter=32, stepsize=alpha, accel=accel)
            got = xt.cpu().numpy()
            want = _torch_iteration(torch, A64, b, lam, 32, alpha, accel)
            nnz = np.count_nonzero(want)
            print(f"λ = {lam}, accel = {accel}: nnz {nnz} of {N}")
            assert nnz > N // 2 if dense else 0 < nnz < N // 64
            tw.compare(got, want)
            D.ctx.ista_device(b, lam, xt, maxiter=32, stepsize=alpha, accel=accel)
            assert np.array_equal(xt.cpu().numpy(), got)
    D.close()


@pytest.mark.parametrize("lam", [1e-3, 0.2])
@pytest.mark.parametrize("accel", [False, True])
def test_two_runs_give_the_same_bits(cs, lam, accel):
    A, _, b, alpha, _ = tw.case_data("512x4096_f32")
    D = cs.Dictionary(A)
    x1, r1 = D.ctx.ista(b, lam, maxiter=300, stepsize=alpha, accel=accel)
    x2, r2 = D.ctx.ista(b, lam, maxiter=300, stepsize=alpha, accel=accel)
    D.close()
    D = cs.Dictionary(A)  # (and from a fresh context)
    x3, r3 = D.ctx.ista(b, lam, maxiter=300, stepsize=alpha, accel=accel)
    D.close()
    print(f"λ = {lam}: nnz {np.count_nonzero(x1)} of {len(x1)}")
    assert np.array_equal(x1, x2) and np.array_equal(x1, x3) and r1 == r2 == r3


# ------------------------------------------------------------------------------------------ errors
def _raw(L, ctx, b, w, idx0, val0, maxiter, stepsize, accel=0, x=None, nw=None, nnz0=None):
    x = np.zeros(max(ctx.N, 1)) if x is None else x
    rn = C.c_double(0)
    return L.lib().csmp_ista(ctx._h, L.ptr(b), L.dtype_code(b.dtype), L.ptr(w), L.i64(len(w) if nw is None else nw), L.ptr(idx0), L.ptr(val0),
                             L.i64((0 if idx0 is None else len(idx0)) if nnz0 is None else nnz0), L.i64(maxiter), C.c_double(stepsize), accel,
                             L.ptr(x), L.HOST, C.byref(rn))


def test_errors(cs):
    L = cs._lib
    A, _, b, alpha, _ = tw.case_data("32x48_f64")
    N = A.shape[1]
    one = np.array([0.1])
    ctx = cs.Context(0)
    assert _raw(L, ctx, b, one, None, None, 4, alpha) == L.ESTATE  # no dictionary set
    ctx.close()
    D = cs.Dictionary(A, streamed=True)
    assert _raw(L, D.ctx, b, one, None, None, 4, alpha) == L.ESTATE  # a host-streamed dictionary
    assert "streamed" in L.lib().csmp_last_error(D.ctx._h).decode()
    D.close()
    D = cs.Dictionary(A)
    ctx = D.ctx
    for nw in (0, 2, N - 1, N + 1):
        assert _raw(L, ctx, b, np.full(N + 1, 0.1), None, None, 4, alpha, nw=nw) == L.EDIM, nw
    assert _raw(L, ctx, b, one, None, None, -1, alpha) == L.EINVAL
    for bad in (0.0, -1e-2, float("inf"), float("nan")):
        assert _raw(L, ctx, b, one, None, None, 4, bad) == L.EINVAL, bad
    for bad in (-1e-3, float("inf"), float("nan")):
        assert _raw(L, ctx, b, np.array([bad]), None, None, 4, alpha) == L.EINVAL, bad
        w = np.full(N, 0.1)
        w[N // 2] = bad
        assert _raw(L, ctx, b, w, None, None, 4, alpha) == L.EINVAL, bad
    v3 = np.ones(3)
    for idx in ([0, 1, N], [-1, 2, 3], [4, 9, 4]):  # out of range (both ends), repeated
        assert _raw(L, ctx, b, one, np.array(idx, np.int64), v3, 4, alpha) == L.EINVAL, idx
    assert _raw(L, ctx, b, one, None, None, 4, alpha, accel=2) == L.EINVAL
    assert _raw(L, ctx, b, one, None, None, 4, alpha, nnz0=-1) == L.EINVAL
    x, _ = ctx.ista(b, 0.1, maxiter=8, stepsize=alpha)  # the context still solves
    tw.compare(x, tw.ista(A, b, 0.1, None, 8, alpha))
    with pytest.raises(cs.CsmpError) as e:
        ctx.ista(b[:-1], 0.1)
    assert e.value.code == L.EDIM
    D.close()


# ------------------------------------------------------------------------------------------ allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_leaks.py's pattern: fail_alloc = n makes the n-th device allocation from now fail for real.  Every allocation of an
    ista call fails in turn with CSMP_ENOMEM, the same context then returns the clean context's bits, and the library holds what it
    held before -- after that sequence, and after 50 create / solve / destroy cycles."""
    L = cs._lib
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    gc.collect()
    base = L.live_resources()

    def solve(ctx, accel):
        return ctx.ista(b, 2e-2, maxiter=24, stepsize=alpha, accel=accel)

    for accel in (False, True):
        clean = cs.Dictionary(A)
        want = solve(clean.ctx, accel)
        clean.close()
        n, seen_ok, failed = 0, 0, 0
        while seen_ok < 2 and n < 200:
            n += 1
            d = cs.Dictionary(A)
            d.ctx.tune("fail_alloc", n)
            try:
                got = solve(d.ctx, accel)
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], n
                seen_ok += 1
            except cs.CsmpError as e:
                seen_ok = 0
                failed += 1
                assert e.code == L.ENOMEM, (n, e.code, str(e))
            d.ctx.tune("fail_alloc", 0)
            got = solve(d.ctx, accel)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (n, "after the failed call")
            d.close()
        print(f"accel = {accel}: {failed} allocations failed in turn")
        assert n < 200 and failed >= 8  # (the eight buffers of the iteration, and the solver slot's before them)
        gc.collect()
        assert L.live_resources() == base
    for cycle in range(50):
        d = cs.Dictionary(A)
        solve(d.ctx, cycle % 2 == 1)
        d.close()
    gc.collect()
    assert L.live_resources() == base


def test_other_solvers_are_not_disturbed(cs):
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    eps = float(np.finfo(np.float32).eps)
    D = cs.Dictionary(A)
    before = D.ctx.omp(b, 16, eps)
    mp_before = D.ctx.mp(b, 24)
    x1 = D.ctx.ista(b, 2e-2, maxiter=50, stepsize=alpha)
    after = D.ctx.omp(b, 16, eps)
    x2 = D.ctx.ista(b, 2e-2, maxiter=50, stepsize=alpha, accel=True)
    mp_after = D.ctx.mp(b, 24)
    x3 = D.ctx.ista(b, 2e-2, maxiter=50, stepsize=alpha)
    D.close()
    assert all(np.array_equal(u, v) for u, v in zip(before, after))
    assert all(np.array_equal(u, v) for u, v in zip(mp_before, mp_after))
    assert np.array_equal(x1[0], x3[0]) and x1[1] == x3[1] and x2[0].any()
