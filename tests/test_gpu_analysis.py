"""GPU tests (pytest -m gpu) of the dictionary analysis: csmp_colnorms (src/util.jl:2) and csmp_cumbabel (coherence / babel / cumbabel,
src/util.jl:96-115) against the numpy Float64 twin of tests/analysis_twin.py.  The bound is derived, not measured:
|Δμ₁(m)| ≤ 2 m γ(M + 8) S + 2 γ(m) μ₁(m) with S = max_j ‖a_j‖² (1 under normalize) -- see analysis_twin.tolerance."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(A, got, want, normalize, what):
    tol = tw.tolerance(A, want, normalize)
    err = np.abs(got - want)
    worst = int(np.argmax(err / tol))
    print(f"{what} normalize={int(normalize)}: μ₁(1) = {got[0]:.15e}, μ₁({len(got)}) = {got[-1]:.15e}, "
          f"max |Δ| / bound = {err[worst] / tol[worst]:.3e} at m = {worst + 1}")
    assert np.all(err <= tol), (what, worst + 1, err[worst], tol[worst])


# ------------------------------------------------------------------------------------------ parity with the twin
@pytest.mark.parametrize("case", tw.PARITY_CASES, ids=tw.case_id)
def test_cumbabel_matches_the_twin(cs, case):
    M, N, dt, ks = case
    A = tw.random_dictionary(M, N, dt)
    D = cs.Dictionary(np.asarray(A))
    try:
        for k in ks:
            for normalize in (False, True):
                mu, pair = D.ctx.cumbabel(k, normalize)
                assert mu.shape == (k,) and 0 <= pair[0] < pair[1] < N
                _check(A, mu, tw.case_twin(M, N, dt, k, normalize), normalize, f"{tw.case_id(case)} k={k}")
    finally:
        D.close()


def test_device_resident_dictionary_with_a_padded_stride(cs):
    """70 x 130 Float32 handed over in device memory with ldA = 71: columns that start on no 16-byte boundary"""
    import torch
    L = cs._lib
    M, N, ld = 70, 130, 71
    A = tw.random_dictionary(M, N, "f32")
    buf = np.zeros((N, ld), np.float32)
    buf[:, :M] = np.asarray(A).T
    t = torch.from_numpy(buf).cuda()
    ctx = cs.Context(0)
    try:
        ctx.call("csmp_set_dictionary", L.vp(t.data_ptr()), L.i64(M), L.i64(N), L.i64(ld), L.F32, L.DEVICE)
        ctx.M, ctx.N, ctx.dtype, ctx._keep = M, N, np.dtype(np.float32), t
        for normalize in (False, True):
            mu, pair = ctx.cumbabel(3, normalize)
            _check(A, mu, tw.cumbabel(A, 3, normalize), normalize, "70x130_f32 ldA=71")
        norms = ctx.colnorms()
        assert np.all(np.abs(norms - np.linalg.norm(np.asarray(A, np.float64), axis=0)) <= tw.gamma(M + 2) * norms)
    finally:
        ctx.close()


def test_a_single_column(cs):
    A = np.asfortranarray(np.random.default_rng(3).standard_normal((16, 1)))
    D = cs.Dictionary(A)
    for normalize in (False, True):
        mu, pair = D.ctx.cumbabel(1, normalize)
        assert mu.tolist() == [0.0] and pair == (-1, -1)
    D.close()
    assert cs.coherence(A, return_pair=True) == (0.0, (-1, -1))


# ------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("shape", [(200, 130, "f32"), (64, 300, "f64"), (16, 1500, "f64")], ids=lambda s: f"{s[0]}x{s[1]}_{s[2]}")
@pytest.mark.parametrize("planted", [True, False], ids=["ties", "plain"])
def test_integer_dictionaries_are_exact(cs, shape, planted):
    """entries in {-2..2}: every product and sum is exact in Float64, so μ₁ equals the twin bit for bit, and the pair is the twin's under
    the tie-break -- with duplicated and negated columns planted (several pairs tie) and without.  16 x 1500: rows in which far more
    than 1024 entries equal the k-th largest (the selection fixes all eight bytes and fills up with copies of it)"""
    M, N, dt = shape
    A = tw.integer_dictionary(M, N, dt, 7, planted)
    D = cs.Dictionary(A)
    try:
        for k in (1, 9, min(N, 1024)):
            mu, pair = D.ctx.cumbabel(k, False)
            assert np.array_equal(mu, tw.cumbabel(A, k)), k
            assert pair == tw.pair(A), (pair, tw.pair(A))
        if planted:
            assert pair == (3, 5)
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ the pair on real-valued data
@pytest.mark.parametrize("shape", [(100, 257, "f32"), (64, 300, "f64")], ids=lambda s: f"{s[0]}x{s[1]}_{s[2]}")
def test_pair_of_a_planted_near_duplicate(cs, shape):
    M, N, dt = shape
    A = np.array(tw.random_dictionary(M, N, dt, 5))
    i, j = 131, 17
    A[:, j] = A[:, i] + 1e-3 * np.random.default_rng(9).standard_normal(M).astype(A.dtype) / np.sqrt(M)
    for normalize in (False, True):
        want = tw.cumbabel(A, 1, normalize)
        gap, tol = tw.top1_gap(A, normalize), float(tw.tolerance(A, want, normalize)[0])
        print(f"normalize={int(normalize)}: top-1 gap {gap:.3e}, tolerance {tol:.3e}")
        assert gap > 2 * tol and tw.pair(A, normalize) == (17, 131)  # on the twin alone
        mu, pair = cs.coherence(A, normalize=normalize, return_pair=True)
        assert pair == (17, 131)
        assert abs(mu - want[0]) <= tol


# ------------------------------------------------------------------------------------------ colnorms
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_colnorms(cs, dt):
    import torch
    M, N = 333, 130
    A = np.array(tw.random_dictionary(M, N, dt, 2))
    A[:, 41] = 0.0
    A[:, 7] *= 1e3
    want = np.linalg.norm(A.astype(np.float64), axis=0)
    D = cs.Dictionary(A)
    try:
        host = D.ctx.colnorms()
        dev = D.ctx.colnorms(device=True)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64
        assert host.shape == (N,) and np.array_equal(dev.cpu().numpy(), host)
        err = np.abs(host - want)
        print(f"{dt}: max relative error {np.max(err[want > 0] / want[want > 0]):.3e}, bound {float(tw.gamma(M + 2)):.3e}")
        assert np.all(err <= tw.gamma(M + 2) * want) and host[41] == 0.0
        assert np.array_equal(cs.colnorms(A), host) and np.array_equal(cs.colnorms(D), host)
        # normalize = 1: the zero column's row and column contribute nothing
        mu, pair = D.ctx.cumbabel(N, True)
        _check(A, mu, tw.cumbabel(A, N, True), True, f"333x130_{dt} with a zero column")
        assert np.isfinite(mu).all() and 41 not in pair
        B = np.delete(A, 41, axis=1)
        mub = cs.cumbabel(B, N - 1, normalize=True)
        assert np.array_equal(mu[:N - 1], mub) and mu[N - 1] == mu[N - 2]  # (the zero column adds one more zero to every row)
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ the package
def test_api_functions_agree(cs):
    M, N, dt = 256, 1000, "f32"
    A = np.asarray(tw.random_dictionary(M, N, dt))
    D = cs.Dictionary(A)
    try:
        for normalize in (False, True):
            mu = cs.cumbabel(D, 64, normalize=normalize)
            assert mu.dtype == np.float64 and np.array_equal(mu, D.ctx.cumbabel(64, normalize)[0])
            assert np.array_equal(mu, cs.cumbabel(A, 64, normalize=normalize))
            assert cs.babel(D, 64, normalize=normalize) == mu[63] == cs.babel(A, 64, normalize)
            assert cs.babel(D, 17, normalize=normalize) == mu[16]
            c, pair = cs.coherence(D, normalize=normalize, return_pair=True)
            assert c == mu[0] == cs.coherence(A, normalize) == cs.babel(D, 1, normalize) and pair == tw.pair(A, normalize)
            assert isinstance(c, float)
    finally:
        D.close()


def test_two_runs_give_the_same_bits(cs):
    A = np.asarray(tw.random_dictionary(256, 1000, "f32"))
    D = cs.Dictionary(A)
    r1 = [D.ctx.cumbabel(64, nz) for nz in (False, True)]
    r2 = [D.ctx.cumbabel(64, nz) for nz in (False, True)]
    D.close()
    D = cs.Dictionary(A)  # (and from a fresh context)
    r3 = [D.ctx.cumbabel(64, nz) for nz in (False, True)]
    D.close()
    for a, b, c in zip(r1, r2, r3):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and a[1] == b[1] == c[1]


def test_other_solvers_are_not_disturbed(cs):
    L = cs._lib
    A, _, b = cs.sparse_data(n=256, m=1024, k=16, rng=0, dtype=np.float32)
    eps = float(np.finfo(np.float32).eps)
    alpha = 0.45 / float(np.linalg.norm(A.astype(np.float64), 2)) ** 2
    D = cs.Dictionary(A)
    try:
        omp0 = D.ctx.omp(b, 16, eps)
        ista0 = D.ctx.ista(b, 2e-2, maxiter=30, stepsize=alpha)
        mu0 = D.ctx.cumbabel(32, True)
        n0 = D.ctx.colnorms()
        omp1 = D.ctx.omp(b, 16, eps)
        ista1 = D.ctx.ista(b, 2e-2, maxiter=30, stepsize=alpha)
        mu1 = D.ctx.cumbabel(32, True)
        assert all(np.array_equal(u, v) for u, v in zip(omp0, omp1))
        assert np.array_equal(ista0[0], ista1[0]) and ista0[1] == ista1[1]
        assert np.array_equal(mu0[0], mu1[0]) and mu0[1] == mu1[1]
        # a stepwise solve goes on unchanged after an analysis call in its middle
        D.ctx.solver_begin(L.ALGO_OMP, b, 16)
        for _ in range(16):
            D.ctx.solver_step()
        want = D.ctx.solver_state(16)
        D.ctx.solver_begin(L.ALGO_OMP, b, 16)
        for step in range(16):
            if step == 7:
                assert np.array_equal(D.ctx.cumbabel(32, True)[0], mu0[0]) and np.array_equal(D.ctx.colnorms(), n0)
            D.ctx.solver_step()
        got = D.ctx.solver_state(16)
        assert all(np.array_equal(u, v) for u, v in zip(want, got))
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ errors
def _cumbabel(L, h, k, normalize=0, mu=True, pair=True):
    m = np.zeros(1100)
    p = np.zeros(2, np.int64)
    return L.lib().csmp_cumbabel(h, L.i64(k), normalize, L.ptr(m) if mu else None, L.ptr(p) if pair else None)


def _colnorms(L, h, out=True, loc=None):
    o = np.zeros(4096)
    return L.lib().csmp_colnorms(h, L.ptr(o) if out else None, L.HOST if loc is None else loc)


def test_errors(cs):
    L = cs._lib
    A = np.asarray(tw.random_dictionary(32, 48, "f64"))
    assert _cumbabel(L, None, 1) == L.EINVAL and _colnorms(L, None) == L.EINVAL
    ctx = cs.Context(0)
    assert _cumbabel(L, ctx._h, 1) == L.ESTATE and _colnorms(L, ctx._h) == L.ESTATE  # no dictionary set
    assert _cumbabel(L, ctx._h, 1, mu=False) == L.EINVAL and _colnorms(L, ctx._h, out=False) == L.EINVAL
    ctx.close()
    D = cs.Dictionary(A, streamed=True)
    assert _cumbabel(L, D.ctx._h, 1) == L.ESTATE and "streamed" in L.lib().csmp_last_error(D.ctx._h).decode()
    assert _colnorms(L, D.ctx._h) == L.ESTATE and "streamed" in L.lib().csmp_last_error(D.ctx._h).decode()
    D.close()
    D = cs.Dictionary(A)
    h = D.ctx._h
    try:
        assert _cumbabel(L, h, 1, mu=False) == L.EINVAL
        for bad in (-1, 2, 7):
            assert _cumbabel(L, h, 1, normalize=bad) == L.EINVAL, bad
        assert _colnorms(L, h, out=False) == L.EINVAL
        for bad in (-1, 2, L.HOST_STREAMED + 1):
            assert _colnorms(L, h, loc=bad) == L.EINVAL, bad
        for bad in (0, -1, 49, 1025, 1 << 40):
            assert _cumbabel(L, h, bad) == L.ERANGE, bad
        assert _cumbabel(L, h, 48) == L.OK and _cumbabel(L, h, 48, pair=False) == L.OK and _colnorms(L, h) == L.OK
        with pytest.raises(cs.CsmpError) as e:
            D.ctx.cumbabel(49)
        assert e.value.code == L.ERANGE
        # the cap: k = 1025 is refused whatever N is; the buffers follow a dictionary of another shape
        B = np.asarray(tw.random_dictionary(64, 1500, "f64"))
        D.ctx.set_dictionary(B)
        assert _cumbabel(L, h, 1025) == L.ERANGE and _cumbabel(L, h, 1024) == L.OK
        mu, pair = D.ctx.cumbabel(1024, False)
        assert np.array_equal(mu, _fresh(cs, B, 1024)) and np.array_equal(D.ctx.colnorms(), _fresh_norms(cs, B))
        D.ctx.set_dictionary(A)
        assert np.array_equal(D.ctx.cumbabel(48, True)[0], _fresh(cs, A, 48, True)) and D.ctx.colnorms().shape == (48,)
    finally:
        D.close()


def _fresh(cs, A, k, normalize=False):
    D = cs.Dictionary(A)
    try:
        return D.ctx.cumbabel(k, normalize)[0]
    finally:
        D.close()


def _fresh_norms(cs, A):
    D = cs.Dictionary(A)
    try:
        return D.ctx.colnorms()
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_ista.py's pattern: fail_alloc = n makes the n-th device allocation from now fail for real.  Every allocation of a
    colnorms / cumbabel call fails in turn with CSMP_ENOMEM, the same context then returns the clean context's bits, and the library
    holds what it held before."""
    L = cs._lib
    A = np.asarray(tw.random_dictionary(100, 257, "f32"))
    gc.collect()
    base = L.live_resources()

    def both(ctx):
        return ctx.cumbabel(7, True), ctx.colnorms()

    def same(got, want):
        return np.array_equal(got[0][0], want[0][0]) and got[0][1] == want[0][1] and np.array_equal(got[1], want[1])

    clean = cs.Dictionary(A)
    want = both(clean.ctx)
    clean.close()
    for first in ("cumbabel", "colnorms"):
        n, seen_ok, failed = 0, 0, 0
        while seen_ok < 2 and n < 50:
            n += 1
            d = cs.Dictionary(A)
            d.ctx.tune("fail_alloc", n)
            try:
                if first == "colnorms":
                    assert np.array_equal(d.ctx.colnorms(), want[1]), n
                assert same(both(d.ctx), want), n
                seen_ok += 1
            except cs.CsmpError as e:
                seen_ok = 0
                failed += 1
                assert e.code == L.ENOMEM, (n, e.code, str(e))
            d.ctx.tune("fail_alloc", 0)
            assert same(both(d.ctx), want), (n, "after the failed call")
            d.close()
        print(f"{first} first: {failed} allocations failed in turn")
        assert n < 50 and failed >= 7  # the norms, the strip, the three per-row arrays, mu, the best pair
        gc.collect()
        assert L.live_resources() == base
    for cycle in range(20):
        d = cs.Dictionary(A)
        both(d.ctx)
        d.close()
    gc.collect()
    assert L.live_resources() == base
