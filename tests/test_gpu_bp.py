"""GPU tests of basis pursuit on the device: k_rowgram alone (through csmp_bp_rowgram), csmp_bp and csmp_bp_reweighted against the numpy
twin (tests/bp_twin.py), the kept factor, the refusals, device pointers, and allocation failures."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as tw  # noqa: E402
import ista_twin as it_tw  # noqa: E402
import reweight_twin as rt  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


# ------------------------------------------------------------------------------------------ k_rowgram
# M under one 128-row tile, M ragged, M over one and over two tiles, and an N that no split or stage divides.  The column split engages
# from N = 512 on (two splits of at least 256 columns): (130, 1000) runs three splits, (64, 4100) sixteen.
ROWGRAM_SHAPES = [(32, 48), (100, 257), (130, 1000), (257, 300), (64, 4100)]


def _check_gram(G, A, what):
    A64 = np.asarray(A, dtype=np.float64)
    M, N = A64.shape
    ref = A64 @ A64.T
    bound = 2 * (N + 2) * U * (np.abs(A64) @ np.abs(A64).T)  # two summation orders of N products
    err = np.abs(G - ref)
    print(f"{what}: max |G - ref| / bound = {np.max(err / bound):.3e}")
    assert G.shape == (M, M)
    assert np.all(err <= bound), np.argwhere(err > bound)[:5]
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", ROWGRAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rowgram(cs, shape, dtype):
    M, N = shape
    A, _, _ = tw.data(M, N, 3, 11, dtype)
    D = cs.Dictionary(A)
    try:
        G = D.ctx.bp_rowgram()
        _check_gram(G, A, f"{M}x{N} {np.dtype(dtype).name}")
        assert np.array_equal(D.ctx.bp_rowgram(), G)  # the same bits on a second run
        assert np.array_equal(D.ctx.bp_rowgram(device=True).cpu().numpy(), G)
    finally:
        D.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(100, 257), (130, 1000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rowgram_without_16_byte_loads(cs, shape, dtype):
    """k_rowgram's scalar-load instantiation, the one for columns that start on no 16-byte boundary.  A dictionary handed over in device
    memory with ldA = M + 1 is such a pointer, but the library copies what it cannot borrow into 16-byte columns of its own: the
    instantiation is reached through csmp_tune(CSMP_TUNE_ROWGRAM_SCALAR) -- and both must give the bits of the 16-byte path."""
    import torch
    L = cs._lib
    M, N = shape
    ld = M + 1
    A, _, _ = tw.data(M, N, 3, 12, dtype)
    buf = np.zeros((N, ld), dtype)
    buf[:, :M] = np.asarray(A).T
    t = torch.from_numpy(buf).cuda()
    ctx = cs.Context(0)
    D = cs.Dictionary(A)
    try:
        want = D.ctx.bp_rowgram()
        b = np.asarray(A, np.float64) @ np.r_[1.0, -1.0, np.zeros(N - 2)]
        x, info = D.ctx.bp(b, maxiter=512)
        assert info["converged"]
        ctx.call("csmp_set_dictionary", L.vp(t.data_ptr()), L.i64(M), L.i64(N), L.i64(ld), L.dtype_code(np.dtype(dtype)), L.DEVICE)
        ctx.M, ctx.N, ctx.dtype, ctx._keep = M, N, np.dtype(dtype), t
        for c in (ctx, D.ctx):
            c.tune("rowgram_scalar", 1)
            G = c.bp_rowgram()
            _check_gram(G, A, f"{M}x{N} {np.dtype(dtype).name} scalar loads")
            assert np.array_equal(G, want)
        x2, info2 = ctx.bp(b, maxiter=512)  # (factorises the scalar path's G)
        assert np.array_equal(x, x2) and info == info2
    finally:
        ctx.close()
        D.close()


# ------------------------------------------------------------------------------------------ recovery, parity
def test_recovery_of_the_reference_test(cs):
    """test/basispursuit.jl:13-23: at 32 x 48, k = 3, bp, bp_candes and bp_ard recover the support of x0"""
    for seed in (0, 1, 2):
        A, x0, b = tw.data(32, 48, 3, seed)
        D = cs.Dictionary(A)
        try:
            for name, fn in (("bp", cs.bp), ("bp_candes", cs.bp_candes), ("bp_ard", cs.bp_ard)):
                x = fn(D, b)
                err = float(np.max(np.abs(x.to_dense() - x0)))
                print(f"seed {seed} {name}: nnz {x.nnz}, max|x - x0| = {err:.3e}")
                assert np.array_equal(x.nzind, np.flatnonzero(x0)), name
                assert err <= 1e-6, name
        finally:
            D.close()


def _resnorm_bound(A, z, b):
    A64 = np.asarray(A, dtype=np.float64)
    return 2 * (np.count_nonzero(z) + 2) * U * float(np.linalg.norm(np.abs(A64) @ np.abs(z) + np.abs(b)))


@pytest.mark.parametrize("name", sorted(tw.CASES))
def test_parity_with_the_twin(cs, name):
    A, _, b, w = tw.case_data(name)
    zt, it = tw.case_twin(name)
    D = cs.Dictionary(A)
    try:
        z, info = D.ctx.bp(b, 1.0 if w is None else w, tol=tw.TWIN_TOL)
    finally:
        D.close()
    err = float(np.max(np.abs(z - zt)))
    rn = float(np.linalg.norm(np.asarray(A, np.float64) @ z - b))
    print(f"{name}: iterations {info['iterations']} (twin {it['iterations']}), nnz {np.count_nonzero(z)} (twin {np.count_nonzero(zt)}), "
          f"max|z - twin| = {err:.3e}, resnorm {info['resnorm']:.3e} (numpy {rn:.3e}), ||b|| = {np.linalg.norm(b):.3e}")
    assert info["converged"] and it["converged"]
    assert np.array_equal(np.flatnonzero(z), np.flatnonzero(zt))
    assert err <= tw.RTOL * np.max(np.abs(zt))
    assert info["iterations"] <= it["iterations"] + 2 * 32
    assert rn <= 1e-7 * np.linalg.norm(b)
    assert abs(rn - info["resnorm"]) <= _resnorm_bound(A, z, b)


@pytest.mark.parametrize("scheme", ["candes", "ard"])
def test_reweighted_parity_with_the_twin(cs, scheme):
    A, x0, b, _ = tw.case_data("wide_130x1000")
    zt, wt, done_t = tw.bp_reweighted(A, b, scheme, outer_maxiter=3, min_decrease=0.0)
    D = cs.Dictionary(A)
    try:
        z, rn, done, w = D.ctx.bp_reweighted(b, scheme, outer_maxiter=3, min_decrease=0.0, return_weights=True)
        early = D.ctx.bp_reweighted(b, scheme, outer_maxiter=8, min_decrease=1e-3)
    finally:
        D.close()
    print(f"{scheme}: max|z - twin| = {np.max(np.abs(z - zt)):.3e}, max rel |w - twin| = {np.max(np.abs(w - wt) / wt):.3e}, early stop after {early[2]}")
    assert done == done_t == 3
    assert np.array_equal(np.flatnonzero(z), np.flatnonzero(zt)) and np.max(np.abs(z - zt)) <= tw.RTOL * np.max(np.abs(zt))
    assert np.max(np.abs(w - wt) / wt) <= 1e-6
    assert early[2] == 2 and np.array_equal(np.flatnonzero(early[0]), np.flatnonzero(x0))  # x0 is recovered at once: the second solve moves nothing


# ------------------------------------------------------------------------------------------ the factor, interleaving
def test_the_factor_is_kept(cs):
    A, _, b, _ = tw.case_data("recover_32x48")
    D = cs.Dictionary(A)
    try:
        x1, i1 = D.ctx.bp(b)
        x2, i2 = D.ctx.bp(b)
        assert i1["factored"] and not i2["factored"]
        assert np.array_equal(x1, x2) and i1["iterations"] == i2["iterations"] and i1["resnorm"] == i2["resnorm"]
        D.ctx.set_dictionary(A)
        x3, i3 = D.ctx.bp(b)
        assert i3["factored"] and np.array_equal(x1, x3)
        _, r1, d1 = D.ctx.bp_reweighted(b, "candes", outer_maxiter=2)[:3]
        assert not D.ctx.bp(b)[1]["factored"]
    finally:
        D.close()


def test_interleaving_with_ista(cs):
    A, _, b, alpha, _ = it_tw.case_data("256x1024_f32")
    D = cs.Dictionary(A)
    try:
        a1 = D.ctx.ista(b, 2e-2, maxiter=64, stepsize=alpha)
        z1 = D.ctx.bp(b, maxiter=128)
        a2 = D.ctx.ista(b, 2e-2, maxiter=64, stepsize=alpha)
        z2 = D.ctx.bp(b, maxiter=128)
        assert np.array_equal(a1[0], a2[0]) and a1[1] == a2[1]
        assert np.array_equal(z1[0], z2[0])
        c1 = D.ctx.ista_reweighted(b, rt.LAMBDA, "candes", outer_maxiter=2, min_decrease=0.0, maxiter=64, stepsize=alpha, return_weights=True)
        D.ctx.bp_reweighted(b, "candes", outer_maxiter=2, min_decrease=0.0, maxiter=128)
        c2 = D.ctx.ista_reweighted(b, rt.LAMBDA, "candes", outer_maxiter=2, min_decrease=0.0, maxiter=64, stepsize=alpha, return_weights=True)
        assert all(np.array_equal(u, v) for u, v in zip(c1, c2))
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(cs):
    L = cs._lib
    A, _, b, _ = tw.case_data("recover_32x48")
    M, N = A.shape
    D = cs.Dictionary(A)
    want = D.ctx.bp(b)[0]

    def refused(code, text, fn):
        with pytest.raises(cs.CsmpError) as e:
            fn()
        assert e.value.code == code and text in str(e.value), (code, str(e.value))
        assert np.array_equal(D.ctx.bp(b)[0], want)  # the context still solves

    try:
        refused(L.EINVAL, "weights", lambda: D.ctx.bp(b, -np.ones(N)))
        refused(L.EINVAL, "weights", lambda: D.ctx.bp(b, np.r_[np.ones(N - 1), np.inf]))
        refused(L.EINVAL, "weights", lambda: D.ctx.bp(b, np.nan))
        refused(L.EDIM, "length(w)", lambda: D.ctx.bp(b, np.ones(N - 1)))
        refused(L.EINVAL, "rho", lambda: D.ctx.bp(b, rho=0.0))
        refused(L.EINVAL, "rho", lambda: D.ctx.bp(b, rho=-1.0))
        refused(L.EINVAL, "tol", lambda: D.ctx.bp(b, tol=0.0))
        refused(L.EINVAL, "tol", lambda: D.ctx.bp(b, tol=float("nan")))
        refused(L.EINVAL, "check_every", lambda: D.ctx.bp(b, check_every=0))
        refused(L.EINVAL, "rho", lambda: D.ctx.bp_reweighted(b, "candes", rho=0.0))
        refused(L.EINVAL, "scheme", lambda: D.ctx.bp_reweighted(b, 7))
        # more rows than columns
        D.ctx.set_dictionary(np.asfortranarray(A.T))
        with pytest.raises(cs.CsmpError) as e:
            D.ctx.bp(np.ones(N))
        assert e.value.code == L.EDIM
        with pytest.raises(cs.CsmpError) as e:
            D.ctx.bp_reweighted(np.ones(N), "ard")
        assert e.value.code == L.EDIM
        # a repeated row: A A' is singular
        R = np.array(A)
        R[5] = R[3]
        D.ctx.set_dictionary(np.asfortranarray(R))
        for _ in range(2):  # (the verdict is kept with the factor)
            with pytest.raises(cs.CsmpError) as e:
                D.ctx.bp(R @ np.r_[1.0, np.zeros(N - 1)])
            assert e.value.code == L.EINVAL and "bp: A A' is not positive definite to working precision" in str(e.value)
        with pytest.raises(ValueError):
            cs.bp(D, R @ np.r_[1.0, np.zeros(N - 1)])
        D.ctx.set_dictionary(A)
        x, info = D.ctx.bp(b)
        assert info["factored"] and np.array_equal(x, want)
    finally:
        D.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        for fn in (lambda: S.ctx.bp(b), lambda: S.ctx.bp_reweighted(b, "candes"), lambda: S.ctx.bp_rowgram()):
            with pytest.raises(cs.CsmpError) as e:
                fn()
            assert e.value.code == L.ESTATE
    finally:
        S.close()


def test_maxiter_reached_is_no_error(cs):
    A, _, b, _ = tw.case_data("vertex_32x64")
    x, info = cs.bp(A, b, maxiter=32, return_info=True)
    assert info["iterations"] == 32 and not info["converged"] and info["factored"]
    zt, _ = tw.bp(A, b, maxiter=32)
    assert np.max(np.abs(x.to_dense() - zt)) <= tw.RTOL * np.max(np.abs(zt))
    x0, info0 = cs.bp(A, b, maxiter=0, return_info=True)
    assert x0.nnz == 0 and info0["iterations"] == 0 and not info0["converged"] and info0["resnorm"] == pytest.approx(np.linalg.norm(b), rel=1e-14)


# ------------------------------------------------------------------------------------------ device pointers
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["b_f32", "b_f64"])
def test_device_pointers(cs, dtype):
    import torch
    A, _, b, w = tw.case_data("weighted_100x257")
    N = A.shape[1]
    D = cs.Dictionary(A)
    try:
        bh = b.astype(dtype)
        D.ctx.bp(bh, w, maxiter=0)  # (the call that factorises)
        want, winfo = D.ctx.bp(bh, w, maxiter=256)
        bt = torch.from_numpy(bh).cuda()
        xt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        info = D.ctx.bp_device(bt, w, xt, maxiter=256)
        assert np.array_equal(xt.cpu().numpy(), want) and info == winfo and not info["factored"]
        for scheme in ("candes", "ard"):
            rw = D.ctx.bp_reweighted(bh, scheme, outer_maxiter=2, min_decrease=0.0, maxiter=256, return_weights=True)
            wt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
            rn, done = D.ctx.bp_reweighted_device(bt, scheme, xt, wt, outer_maxiter=2, min_decrease=0.0, maxiter=256)
            assert np.array_equal(xt.cpu().numpy(), rw[0]) and rn == rw[1] and done == rw[2] == 2 and np.array_equal(wt.cpu().numpy(), rw[3])
            rn2, _ = D.ctx.bp_reweighted_device(bt, scheme, xt, None, outer_maxiter=2, min_decrease=0.0, maxiter=256)
            assert rn2 == rn and np.array_equal(xt.cpu().numpy(), rw[0])
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_reweight.py's pattern: every device allocation of a bp call fails in turn with CSMP_ENOMEM, the same context then
    returns the clean context's bits, and the library holds what it held before."""
    L = cs._lib
    A, _, b, _ = tw.case_data("recover_32x48")
    gc.collect()
    base = L.live_resources()

    def solve(ctx):
        x, info = ctx.bp(b)
        return x, np.array([info["iterations"], info["converged"], info["resnorm"]])

    def reweighted(ctx):
        return ctx.bp_reweighted(b, "ard", ard_iter=2, outer_maxiter=2, min_decrease=0.0, return_weights=True)

    def gram(ctx):
        return (ctx.bp_rowgram(),)

    # bp: the 8 buffers of the iterates, the 8 of G and its factor, the partials of k_rowgram (after the solver slot's); the hook: the
    # partials and the matrix
    for call, least in ((solve, 17), (reweighted, 17 + 19), (gram, 2)):
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
    for _ in range(20):
        d = cs.Dictionary(A)
        d.ctx.bp(b)
        d.close()
    gc.collect()
    assert L.live_resources() == base
