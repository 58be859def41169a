"""GPU tests of sparse Bayesian learning on the device: the weighted k_rowgram alone (csmp_sbl_rowgram), k_sbl_forms alone on directions of
the test's own (csmp_sbl_forms), csmp_sbl against the numpy twin (tests/sbl_twin.py), the step form, the refusals, device pointers, the
other solvers' kept state, and allocation failures."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as bt  # noqa: E402
import bpd_twin as bdt  # noqa: E402
import ista_twin as it_tw  # noqa: E402
import sbl_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
S2 = tw.SIGMA ** 2


# ------------------------------------------------------------------------------------------ the weighted k_rowgram
# tests/test_gpu_bp.py's shapes: M under one 128-row tile, M ragged, M over one and over two tiles, and an N that no split or stage divides
ROWGRAM_SHAPES = [(32, 48), (100, 257), (130, 1000), (257, 300), (64, 4100)]


def _gamma(N, seed):
    """entries spread over 1e-14 .. 1e2, both ends present"""
    g = 10.0 ** np.random.default_rng(seed).uniform(-14.0, 2.0, N)
    g[0], g[-1] = 1e-14, 1e2
    return g


def _check_gram(G, A, g, what):
    """test_gpu_bp.py's _check_gram with |γ| inside: two summation orders of N products, each with one rounding more (the scaling)"""
    A64 = np.asarray(A, dtype=np.float64)
    M, N = A64.shape
    ref = (A64 * g) @ A64.T
    bound = 2 * (N + 3) * U * ((np.abs(A64) * np.abs(g)) @ np.abs(A64).T)
    err = np.abs(G - ref)
    print(f"{what}: max |G - ref| / bound = {np.max(err / bound):.3e}")
    assert G.shape == (M, M)
    assert np.all(err <= bound), np.argwhere(err > bound)[:5]
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", ROWGRAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_weighted_rowgram(cs, shape, dtype):
    import torch
    M, N = shape
    A, _, _ = bt.data(M, N, 3, 11, dtype)
    g = _gamma(N, 21)
    D = cs.Dictionary(A)
    try:
        G = D.ctx.sbl_rowgram(g)
        _check_gram(G, A, g, f"{M}x{N} {np.dtype(dtype).name}")
        assert np.array_equal(D.ctx.sbl_rowgram(g), G)  # the same bits on a second run
        assert np.array_equal(D.ctx.sbl_rowgram(torch.from_numpy(g).cuda(), device=True).cpu().numpy(), G)
        D.ctx.tune("sbl_scalar", 1)  # the scalar-load instantiation gives the bits of the 16-byte one
        assert np.array_equal(D.ctx.sbl_rowgram(g), G)
        D.ctx.tune("sbl_scalar", 0)
        G1 = D.ctx.sbl_rowgram(np.ones(N))
        _check_gram(G1, A, np.ones(N), f"{M}x{N} {np.dtype(dtype).name} γ = 1")
        A64 = np.asarray(A, np.float64)
        assert np.all(np.abs(G1 - D.ctx.bp_rowgram()) <= 2 * (N + 3) * U * (np.abs(A64) @ np.abs(A64).T))
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ k_sbl_forms
# M = 32: under one row block; 100: ragged; 130: two direction blocks, the second with 2 directions -- the smallest shape at which the skip
# engages --; 257: three direction blocks, five row blocks.  N = 48, 257, 300: the last workgroup holds fewer than 128 atoms.
FORMS_SHAPES = [(32, 48), (100, 257), (130, 300), (257, 300)]


def _directions(M, seed):
    """a dense upper triangular W (every entry of the triangle non-zero), with whole 64-row blocks of rows, and a dense t"""
    rng = np.random.default_rng(seed)
    ldw = (M + 63) // 64 * 64
    W = np.zeros((ldw, M), order="F")
    W[:M] = np.triu(rng.uniform(0.5, 1.5, (M, M)) * rng.choice(np.array([-1.0, 1.0]), (M, M))) / np.sqrt(M)
    assert np.all(W[:M][np.triu_indices(M)] != 0.0)
    return W, rng.standard_normal(M)


def _forms_bounds(A, W, t):
    """p_d = Σ_i W[i, d] a_i is a sum of at most M products: two summation orders put the kernel's p_d within
    e_d = 2 (M + 2) u Σ_i |W[i, d]| |a_i| of numpy's.  s = Σ_d p_d² and q = Σ_d p_d t_d then differ by the propagated e_d,
    e_d (2 |p_d| + e_d) resp. e_d |t_d|, plus two summation orders of M terms of the sums themselves."""
    A64 = np.asarray(A, dtype=np.float64)
    M = A64.shape[0]
    P = W[:M].T @ A64
    e = 2 * (M + 2) * U * (np.abs(W[:M]).T @ np.abs(A64))
    Pa = np.abs(P) + e
    bs = np.sum(e * (2 * np.abs(P) + e), axis=0) + 2 * (M + 2) * U * np.sum(Pa * Pa, axis=0)
    bq = np.abs(t) @ e + 2 * (M + 2) * U * (np.abs(t) @ Pa)
    return np.sum(P * P, axis=0), P.T @ t, bs, bq


@pytest.mark.parametrize("scalar", [0, 1], ids=["vec", "scalar"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", FORMS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forms(cs, shape, dtype, scalar):
    M, N = shape
    A, _, _ = bt.data(M, N, 3, 13, dtype)
    W, t = _directions(M, 31)
    s_ref, q_ref, bs, bq = _forms_bounds(A, W, t)
    D = cs.Dictionary(A)
    try:
        D.ctx.tune("sbl_scalar", scalar)
        s, q = D.ctx.sbl_forms(W, t)
        print(f"{M}x{N} {np.dtype(dtype).name}: max |s - ref| / bound = {np.max(np.abs(s - s_ref) / bs):.3e}, "
              f"max |q - ref| / bound = {np.max(np.abs(q - q_ref) / bq):.3e}")
        assert np.all(np.abs(s - s_ref) <= bs) and np.all(np.abs(q - q_ref) <= bq)
        s2, q2 = D.ctx.sbl_forms(W, t)
        assert np.array_equal(s, s2) and np.array_equal(q, q2)  # the same bits on a second run
        # the skip: the row blocks the kernel documents as never read -- from row 128 (D + 1) on in direction block D -- hold NaN
        Wn = np.array(W, order="F")
        for Dblk in range((M + 127) // 128):
            Wn[128 * (Dblk + 1):, 128 * Dblk:128 * (Dblk + 1)] = np.nan
        assert bool(np.isnan(Wn).any()) == (M > 128)
        sn, qn = D.ctx.sbl_forms(Wn, t)
        assert not np.isnan(sn).any() and not np.isnan(qn).any()
        assert np.array_equal(sn, s) and np.array_equal(qn, q)
        # ... and inside the blocks that are read, what lies below the diagonal does not count
        Wl = np.array(W, order="F")
        Wl[:M][np.tril_indices(M, -1)] = np.nan
        Wl[M:] = np.nan
        sl, ql = D.ctx.sbl_forms(Wl, t)
        assert np.array_equal(sl, s) and np.array_equal(ql, q)
    finally:
        D.close()


def test_forms_scalar_loads_give_the_same_bits(cs):
    for M, N in ((100, 257), (257, 300)):
        A, _, _ = bt.data(M, N, 3, 14, np.float32)
        W, t = _directions(M, 32)
        D = cs.Dictionary(A)
        try:
            a = D.ctx.sbl_forms(W, t)
            D.ctx.tune("sbl_scalar", 1)
            b = D.ctx.sbl_forms(W, t)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        finally:
            D.close()


# ------------------------------------------------------------------------------------------ parity, recovery
@pytest.mark.parametrize("name", sorted(tw.CASES))
def test_parity_with_the_twin(cs, name):
    """the project's parity contract: the same number of updates, converged, x and γ within 1e-6 of the twin's largest entry"""
    A, x0, b, y = tw.case_data(name)
    xt, it = tw.case_twin(name)
    D = cs.Dictionary(A)
    try:
        x, info, g = D.ctx.sbl(y, S2, return_gamma=True)
    finally:
        D.close()
    ex, eg = float(np.max(np.abs(x - xt))), float(np.max(np.abs(g - it["gamma"])))
    print(f"{name}: updates {info['iterations']} (twin {it['iterations']}), max|x - twin| = {ex:.3e} (max|x| = {np.max(np.abs(xt)):.3e}), "
          f"max|γ - twin| = {eg:.3e} (max γ = {np.max(it['gamma']):.3e})")
    assert info["iterations"] == it["iterations"]
    assert info["converged"] and it["converged"]
    assert ex <= tw.RTOL * np.max(np.abs(xt))
    assert eg <= tw.RTOL * np.max(it["gamma"])
    assert tw.recovers(A, x, x0, b)


def test_recovery_of_the_reference_test(cs):
    """test/sbl.jl:7-17: 32 x 48, k = 3, σ = 1e-2, y = perturb(b, σ / 2): the entries above σ are the planted support, A x ≈ b to σ"""
    for seed in (0, 1, 2):
        A, x0, b = cs.sparse_data(32, 48, 3, rng=seed)
        y = cs.perturb(b, tw.SIGMA / 2, rng=100 + seed)
        x = cs.sbl(A, y, S2)
        print(f"seed {seed}: support {np.flatnonzero(np.abs(x) > tw.SIGMA)}, ‖A x − b‖ = {np.linalg.norm(A @ x - b):.3e}")
        assert np.array_equal(np.flatnonzero(np.abs(x) > tw.SIGMA), x0.nzind)
        assert np.linalg.norm(A @ x - b) <= tw.SIGMA


# ------------------------------------------------------------------------------------------ step form, repeatability
def test_step_form(cs):
    A, _, _, y = tw.case_data("100x257_f32")
    D = cs.Dictionary(A)
    S = cs.SBL(D, y, S2)
    try:
        want, winfo = cs.sbl(D, y, S2, maxiter=3, min_change=0.0, return_info=True)
        assert winfo["iterations"] == 3 and not winfo["converged"]
        for _ in range(3):
            x = S()
        assert S.iterations == 3
        assert np.array_equal(x, want) and np.array_equal(S.gamma.cpu().numpy(), winfo["gamma"])
        out = np.zeros(A.shape[1])
        assert S.update_(out) is out  # update!(S, x) fills x
        # gamma_in from a previous call resumes it
        x2, _, g2 = D.ctx.sbl(y, S2, maxiter=2, min_change=0.0, return_gamma=True)
        x3, i3, g3 = D.ctx.sbl(y, S2, maxiter=1, min_change=0.0, gamma=g2, return_gamma=True)
        assert i3["iterations"] == 1 and np.array_equal(x3, want) and np.array_equal(g3, winfo["gamma"])
        x4, i4, g4 = D.ctx.sbl(y, S2, gamma=g3, return_gamma=True)  # ... up to convergence: the whole solve's bits
        xa, ia, ga = D.ctx.sbl(y, S2, return_gamma=True)
        assert i4["converged"] and i4["iterations"] + 3 == ia["iterations"] and np.array_equal(x4, xa) and np.array_equal(g4, ga)
    finally:
        S.close()
        D.close()


def test_two_runs_give_the_same_bits(cs):
    A, _, _, y = tw.case_data("130x1000_f32")
    D = cs.Dictionary(A)
    try:
        a = D.ctx.sbl(y, S2, return_gamma=True)
        b = D.ctx.sbl(y, S2, return_gamma=True)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    finally:
        D.close()
    D = cs.Dictionary(A)
    try:
        c = D.ctx.sbl(y, S2, return_gamma=True)
        assert np.array_equal(a[0], c[0]) and a[1] == c[1] and np.array_equal(a[2], c[2])
    finally:
        D.close()


def test_maxiter_reached_is_no_error(cs):
    A, _, _, y = tw.case_data("32x48_f64")
    x, info = cs.sbl(A, y, S2, maxiter=2, return_info=True)
    assert info["iterations"] == 2 and not info["converged"]
    xt, it = tw.sbl(A, y, S2, maxiter=2)
    assert np.max(np.abs(x - xt)) <= tw.RTOL * np.max(np.abs(xt))
    assert np.max(np.abs(info["gamma"] - it["gamma"])) <= tw.RTOL * np.max(it["gamma"])


def test_zero_column(cs):
    A, _, _, y = tw.case_data("32x48_f64")
    Z = np.array(A, order="F")
    Z[:, 5] = 0.0
    x, info = cs.sbl(Z, y, S2, return_info=True)
    xt, it = tw.sbl(Z, y, S2)
    assert x[5] == 0.0 and info["gamma"][5] == 1e-14
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(info["gamma"]))
    assert info["iterations"] == it["iterations"] and info["converged"]
    assert np.max(np.abs(x - xt)) <= tw.RTOL * np.max(np.abs(xt))


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(cs):
    import torch
    L = cs._lib
    A, _, _, y = tw.case_data("32x48_f64")
    M, N = A.shape
    D = cs.Dictionary(A)
    want = D.ctx.sbl(y, S2)[0]

    def refused(code, text, fn):
        with pytest.raises(cs.CsmpError) as e:
            fn()
        assert e.value.code == code and text in str(e.value), (code, str(e.value))
        assert np.array_equal(D.ctx.sbl(y, S2)[0], want)  # the context still solves

    try:
        for s2 in (0.0, -1e-4, float("inf"), float("nan")):
            refused(L.EINVAL, "sigma2", lambda: D.ctx.sbl(y, s2))
        refused(L.EINVAL, "min_change", lambda: D.ctx.sbl(y, S2, min_change=-1.0))
        refused(L.EINVAL, "min_change", lambda: D.ctx.sbl(y, S2, min_change=float("nan")))
        refused(L.EINVAL, "maxiter", lambda: D.ctx.sbl(y, S2, maxiter=0))
        for bad in (0.0, -1.0, np.inf, np.nan):
            g = np.ones(N)
            g[7] = bad
            refused(L.EINVAL, "gamma", lambda: D.ctx.sbl(y, S2, gamma=g))
            gt, bt_, xt = torch.from_numpy(g).cuda(), torch.from_numpy(y).cuda(), torch.zeros(N, dtype=torch.float64, device="cuda")
            refused(L.EINVAL, "gamma", lambda: D.ctx.sbl_device(bt_, S2, xt, gt, maxiter=1))
        refused(L.EDIM, "length(gamma)", lambda: D.ctx.sbl(y, S2, gamma=np.ones(N - 1)))
        refused(L.EDIM, "length(b)", lambda: D.ctx.sbl(y[:-1], S2))
        x = np.zeros(N)
        it, fl = L.i64(0), L.C.c_int(0)
        args = (L.C.c_double(S2), L.i64(4), L.C.c_double(1e-6), None)
        refused(L.EINVAL, "bad arguments", lambda: D.ctx.call("csmp_sbl", None, L.F64, *args, L.ptr(x), None, L.HOST, L.C.byref(it), L.C.byref(fl)))
        refused(L.EINVAL, "bad arguments", lambda: D.ctx.call("csmp_sbl", L.ptr(y), L.F64, *args, None, None, L.HOST, L.C.byref(it), L.C.byref(fl)))
        refused(L.EINVAL, "b_dtype", lambda: D.ctx.call("csmp_sbl", L.ptr(y), 7, *args, L.ptr(x), None, L.HOST, L.C.byref(it), L.C.byref(fl)))
        refused(L.EINVAL, "loc", lambda: D.ctx.call("csmp_sbl", L.ptr(y), L.F64, *args, L.ptr(x), None, 7, L.C.byref(it), L.C.byref(fl)))
        D.ctx.call("csmp_sbl", L.ptr(y), L.F64, *args, L.ptr(x), None, L.HOST, None, None)  # iterations, flags and gamma_out may be NULL
        with pytest.raises(NotImplementedError) as e:
            cs.sbl(D, y, S2 * np.eye(M))
        assert "a noise covariance matrix Σ is not served: scalar σ² only" in str(e.value)
        with pytest.raises(NotImplementedError):
            cs.SBL(D, y, S2 * np.eye(M))
        refused(L.EDIM, "ldw", lambda: D.ctx.sbl_forms(np.zeros((M, M), order="F"), np.zeros(M)))
    finally:
        D.close()
    # a failed pivot has csmp_bp's status: more rows than columns and no noise to speak of -- A Γ Aᵀ has rank 32 of 48
    At, _, _, yt = tw.case_data("48x32_f64")
    T = cs.Dictionary(At)
    try:
        with pytest.raises(cs.CsmpError) as e:
            T.ctx.sbl(yt, 1e-300)
        assert e.value.code == L.EINVAL and "sbl: sigma2 I + A Gamma A' is not positive definite to working precision" in str(e.value)
        assert T.ctx.sbl(yt, S2)[1]["converged"]  # the context still solves
    finally:
        T.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        for fn in (lambda: S.ctx.sbl(y, S2), lambda: S.ctx.sbl_rowgram(np.ones(N)), lambda: S.ctx.sbl_forms(*_directions(M, 1))):
            with pytest.raises(cs.CsmpError) as e:
                fn()
            assert e.value.code == L.ESTATE
    finally:
        S.close()
    c = cs.Context(0)
    try:
        c.M, c.N = M, N
        with pytest.raises(cs.CsmpError) as e:
            c.sbl(y, S2)
        assert e.value.code == L.ESTATE and "no dictionary" in str(e.value)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------ device pointers
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["b_f32", "b_f64"])
def test_device_pointers(cs, dtype):
    import torch
    A, _, _, y = tw.case_data("100x257_f32")
    N = A.shape[1]
    D = cs.Dictionary(A)
    try:
        yh = y.astype(dtype)
        want, winfo, wg = D.ctx.sbl(yh, S2, return_gamma=True)
        yt = torch.from_numpy(yh).cuda()
        xt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        gt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        info = D.ctx.sbl_device(yt, S2, xt, None, gt)
        assert info == winfo and np.array_equal(xt.cpu().numpy(), want) and np.array_equal(gt.cpu().numpy(), wg)
        info = D.ctx.sbl_device(yt, S2, xt)  # gamma_out is optional
        assert info == winfo and np.array_equal(xt.cpu().numpy(), want)
        W, t = _directions(A.shape[0], 5)
        s, q = D.ctx.sbl_forms(W, t)
        sd, qd = D.ctx.sbl_forms(torch.from_numpy(np.ascontiguousarray(W.T)).cuda(), torch.from_numpy(t).cuda(), device=True)
        assert np.array_equal(sd.cpu().numpy(), s) and np.array_equal(qd.cpu().numpy(), q)
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ the other solvers
def test_other_solvers_are_undisturbed(cs):
    A, _, b, alpha, _ = it_tw.case_data("256x1024_f32")
    delta = 1e-2 * float(np.linalg.norm(b))
    D = cs.Dictionary(A)
    try:
        z1, i1 = D.ctx.bp(b, maxiter=128)
        d1, j1 = D.ctx.bpd(b, delta, maxiter=128)
        a1 = D.ctx.ista(b, 2e-2, maxiter=64, stepsize=alpha)
        assert i1["factored"] and j1["factored"]
        s1 = D.ctx.sbl(b, S2, maxiter=2, return_gamma=True)
        z2, i2 = D.ctx.bp(b, maxiter=128)
        d2, j2 = D.ctx.bpd(b, delta, maxiter=128)
        a2 = D.ctx.ista(b, 2e-2, maxiter=64, stepsize=alpha)
        s2 = D.ctx.sbl(b, S2, maxiter=2, return_gamma=True)
        assert not i2["factored"] and not j2["factored"]  # the kept factors are still the kept factors
        assert np.array_equal(z1, z2) and i1["iterations"] == i2["iterations"] and i1["resnorm"] == i2["resnorm"]
        assert np.array_equal(d1, d2) and j1["iterations"] == j2["iterations"] and j1["resnorm"] == j2["resnorm"]
        assert np.array_equal(a1[0], a2[0]) and a1[1] == a2[1]
        assert np.array_equal(s1[0], s2[0]) and s1[1] == s2[1] and np.array_equal(s1[2], s2[2])
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_bp.py's pattern: every device allocation of an sbl call fails in turn with CSMP_ENOMEM, the same context then returns
    the clean context's bits, and the library holds what it held before."""
    L = cs._lib
    A, _, _, y = tw.case_data("32x48_f64")
    M, N = A.shape
    W, t = _directions(M, 3)
    gc.collect()
    base = L.live_resources()

    def solve(ctx):
        x, info, g = ctx.sbl(y, S2, return_gamma=True)
        return x, g, np.array([info["iterations"], info["converged"]])

    def gram(ctx):
        return (ctx.sbl_rowgram(np.ones(N)),)

    def forms(ctx):
        return ctx.sbl_forms(W, t)

    # sbl: the 13 buffers of SblBuf; the hooks: the partials, the matrix and γ; W, t, s and q
    for call, least in ((solve, 13), (gram, 3), (forms, 4)):
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
        d.ctx.sbl(y, S2)
        d.close()
    gc.collect()
    assert L.live_resources() == base
