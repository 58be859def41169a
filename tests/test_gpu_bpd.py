"""GPU tests of basis pursuit denoising on the device: csmp_bpd and csmp_bpd_reweighted against the numpy twin (tests/bpd_twin.py) and
against the problem's optimality conditions, the kept factor beside csmp_bp's, the refusals, device pointers, and allocation failures.

The shapes of the parity cases are those at which the new kernels can go wrong: M = 32 and 48 (under one tile of the factorisation and
one workgroup of the M-vector stage), 100 and 130 (ragged; 130 over one 128-row tile of k_rowgram), 257 (the M-vector stage over two
256-thread workgroups: k_bpd_ball and k_bpd_fold add more than one partial), N = 1000 (several segments of the update)."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as bt  # noqa: E402
import bpd_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KW = dict(rho=tw.RHO, tol=tw.TWIN_TOL, check_every=tw.CHECK_EVERY)


def _resnorm_bound(A, z, b):
    A64 = np.asarray(A, dtype=np.float64)
    return 2 * (np.count_nonzero(z) + 2) * U * float(np.linalg.norm(np.abs(A64) @ np.abs(z) + np.abs(b)))


# ------------------------------------------------------------------------------------------ parity, certificate
# ragged_257x300 (seed 3) is not among the cases whose inputs were checked before the kernels were written; its twin needs 160 iterations
# at ρ = 100 (under the 5000 that would have called for another seed)
@pytest.mark.parametrize("name", tw.CASES)
def test_parity_with_the_twin(cs, name):
    A, _, b, w, delta = tw.case_data(name)
    zt, it = tw.case_twin(name)
    D = cs.Dictionary(A)
    try:
        z, info = D.ctx.bpd(b, delta, 1.0 if w is None else w, **KW)
    finally:
        D.close()
    err = float(np.max(np.abs(z - zt)))
    rn = float(np.linalg.norm(np.asarray(A, np.float64) @ z - b))
    print(f"{name}: iterations {info['iterations']} (twin {it['iterations']}), nnz {np.count_nonzero(z)} (twin {np.count_nonzero(zt)}), "
          f"max|z - twin| = {err:.3e}, resnorm {info['resnorm']:.6e} (numpy {rn:.6e}), δ = {delta:.6e}")
    assert info["converged"] and it["converged"]
    assert np.array_equal(np.flatnonzero(z), np.flatnonzero(zt))
    assert err <= tw.RTOL * np.max(np.abs(zt))
    assert info["iterations"] <= it["iterations"] + 2 * 32
    assert abs(rn - info["resnorm"]) <= _resnorm_bound(A, z, b)
    assert rn <= delta * (1 + 1e-6)
    if name == "zero":
        assert not np.any(z) and info["iterations"] == 32


def test_the_devices_result_passes_the_optimality_certificate(cs):
    A, _, b, w, delta = tw.case_data("wide_130x1000")
    z, info = cs.bpd(A, b, delta, w, return_info=True, **KW)
    feas, on, off = tw.certificate(A, b, delta, w, z.to_dense())
    print(f"wide_130x1000: {info['iterations']} iterations, nnz {z.nnz}; | ||r|| - δ | / δ = {feas:.3e}, on the support {on:.3e}, off it {off:.6f}")
    assert info["converged"]
    assert feas <= 1e-6
    assert on <= 1e-6
    assert off <= 1 + 1e-6


@pytest.mark.parametrize("scheme", ["candes", "ard"])
def test_reweighted_parity_with_the_twin(cs, scheme):
    A, x0, b, _, delta = tw.case_data("wide_130x1000")
    zt, wt, done_t, its = tw.case_reweighted("wide_130x1000", scheme, 3, 0.0)
    _, _, early_t, _ = tw.case_reweighted("wide_130x1000", scheme, 8, 1e-3)
    D = cs.Dictionary(A)
    try:
        z, rn, done, w = D.ctx.bpd_reweighted(b, delta, scheme, outer_maxiter=3, min_decrease=0.0, return_weights=True, **KW)
        early = D.ctx.bpd_reweighted(b, delta, scheme, outer_maxiter=8, min_decrease=1e-3, **KW)
    finally:
        D.close()
    print(f"{scheme}: twin iterations {its}, max|z - twin| = {np.max(np.abs(z - zt)):.3e}, max rel |w - twin| = {np.max(np.abs(w - wt) / wt):.3e}, "
          f"early stop after {early[2]} (twin {early_t})")
    assert done == done_t == 3
    assert np.array_equal(np.flatnonzero(z), np.flatnonzero(zt)) and np.max(np.abs(z - zt)) <= tw.RTOL * np.max(np.abs(zt))
    assert np.max(np.abs(w - wt) / wt) <= 1e-6
    assert early[2] == early_t < 8
    assert np.array_equal(np.flatnonzero(z), np.flatnonzero(x0)) and np.array_equal(np.flatnonzero(early[0]), np.flatnonzero(x0))
    assert rn <= delta * (1 + 1e-6)


def test_public_reweighted_functions_take_the_references_defaults(cs):
    """eps = δ (candes) and δ² (ard), min_decrease = 1e-4: cs.bpd_candes / cs.bpd_ard against the context's call with these spelled out"""
    A, x0, b, _, delta = tw.case_data("recover_32x48")
    D = cs.Dictionary(A)
    try:
        for fn, scheme, eps in ((cs.bpd_candes, "candes", delta), (cs.bpd_ard, "ard", delta ** 2)):
            x, w = fn(D, b, delta, return_weights=True, **KW)
            want = D.ctx.bpd_reweighted(b, delta, scheme, eps=eps, outer_maxiter=8, min_decrease=1e-4, return_weights=True, **KW)
            assert np.array_equal(x.to_dense(), want[0]) and np.array_equal(w, want[3])
            assert np.array_equal(x.nzind, np.flatnonzero(x0)), scheme
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ the other cases
def test_more_rows_than_columns_and_rank_deficient_dictionaries_are_served(cs):
    L = cs._lib
    A, _, b, _, delta = tw.case_data("tall_48x32")
    D = cs.Dictionary(A)
    try:
        with pytest.raises(cs.CsmpError) as e:
            D.ctx.bp(b)
        assert e.value.code == L.EDIM
        z, info = D.ctx.bpd(b, delta, **KW)
        assert info["converged"] and np.linalg.norm(A @ z - b) <= delta * (1 + 1e-6)
        # a repeated row: A A' is singular (bp refuses it), I + A A' is not
        Aw, _, bw, _, dw = tw.case_data("recover_32x48")
        R = np.array(Aw)
        R[5] = R[3]
        br = np.array(bw)
        br[5] = br[3]
        D.ctx.set_dictionary(np.asfortranarray(R))
        with pytest.raises(cs.CsmpError) as e:
            D.ctx.bp(br)
        assert e.value.code == L.EINVAL and "not positive definite" in str(e.value)
        zt, it = tw.bpd(R, br, dw, **KW)
        z, info = D.ctx.bpd(br, dw, **KW)
        print(f"repeated row: iterations {info['iterations']} (twin {it['iterations']}), max|z - twin| = {np.max(np.abs(z - zt)):.3e}")
        assert info["converged"] and it["converged"] and info["factored"]
        assert np.array_equal(np.flatnonzero(z), np.flatnonzero(zt)) and np.max(np.abs(z - zt)) <= tw.RTOL * np.max(np.abs(zt))
    finally:
        D.close()


def test_delta_zero_is_basis_pursuit(cs):
    A, x0, b, w = bt.case_data("recover_32x48")
    D = cs.Dictionary(A)
    try:
        zb, ib = D.ctx.bp(b, tol=tw.TWIN_TOL)
        z, info = D.ctx.bpd(b, 0.0, **KW)
    finally:
        D.close()
    print(f"δ = 0: {info['iterations']} iterations (bp {ib['iterations']}), max|z - bp| = {np.max(np.abs(z - zb)):.3e}")
    assert info["converged"] and ib["converged"]
    assert np.array_equal(np.flatnonzero(z), np.flatnonzero(x0))
    assert np.max(np.abs(z - zb)) <= 1e-6


# ------------------------------------------------------------------------------------------ the factor, interleaving
def test_the_factor_is_kept(cs):
    A, _, b, _, delta = tw.case_data("recover_32x48")
    D = cs.Dictionary(A)
    try:
        x1, i1 = D.ctx.bpd(b, delta, **KW)
        x2, i2 = D.ctx.bpd(b, delta, **KW)
        assert i1["factored"] and not i2["factored"]
        assert np.array_equal(x1, x2) and i1["iterations"] == i2["iterations"] and i1["resnorm"] == i2["resnorm"]  # the same bits on a second run
        D.ctx.set_dictionary(A)
        x3, i3 = D.ctx.bpd(b, delta, **KW)
        assert i3["factored"] and np.array_equal(x1, x3)
        D.ctx.bpd_reweighted(b, delta, "candes", outer_maxiter=2, **KW)
        assert not D.ctx.bpd(b, delta, **KW)[1]["factored"]
    finally:
        D.close()


def test_bp_and_bpd_keep_a_factor_each(cs):
    A, _, b, _, delta = tw.case_data("weighted_100x257")
    D = cs.Dictionary(A)
    try:
        d1 = D.ctx.bpd(b, delta, maxiter=128, **KW)
        p1 = D.ctx.bp(b, maxiter=128)
        d2 = D.ctx.bpd(b, delta, maxiter=128, **KW)
        p2 = D.ctx.bp(b, maxiter=128)
        d3 = D.ctx.bpd(b, delta, maxiter=128, **KW)
        assert d1[1]["factored"] and p1[1]["factored"]
        assert not d2[1]["factored"] and not p2[1]["factored"] and not d3[1]["factored"]
        assert np.array_equal(d1[0], d2[0]) and np.array_equal(d1[0], d3[0]) and d1[1]["resnorm"] == d2[1]["resnorm"] == d3[1]["resnorm"]
        assert np.array_equal(p1[0], p2[0]) and p1[1]["resnorm"] == p2[1]["resnorm"]
        assert np.any(d1[0] != p1[0])  # (two problems, two answers)
        D.ctx.set_dictionary(A)  # a new dictionary invalidates both
        assert D.ctx.bp(b, maxiter=128)[1]["factored"] and D.ctx.bpd(b, delta, maxiter=128, **KW)[1]["factored"]
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(cs):
    L = cs._lib
    A, _, b, _, delta = tw.case_data("recover_32x48")
    M, N = A.shape
    D = cs.Dictionary(A)
    want = D.ctx.bpd(b, delta, **KW)[0]

    def refused(code, text, fn):
        with pytest.raises(cs.CsmpError) as e:
            fn()
        assert e.value.code == code and text in str(e.value), (code, str(e.value))
        assert np.array_equal(D.ctx.bpd(b, delta, **KW)[0], want)  # the context still solves

    try:
        refused(L.EINVAL, "delta", lambda: D.ctx.bpd(b, -1e-3))
        refused(L.EINVAL, "delta", lambda: D.ctx.bpd(b, float("inf")))
        refused(L.EINVAL, "delta", lambda: D.ctx.bpd(b, float("nan")))
        refused(L.EINVAL, "delta", lambda: D.ctx.bpd_reweighted(b, -1.0, "candes", eps=1e-2))
        refused(L.EINVAL, "weights", lambda: D.ctx.bpd(b, delta, -np.ones(N)))
        refused(L.EINVAL, "weights", lambda: D.ctx.bpd(b, delta, np.r_[np.ones(N - 1), np.inf]))
        refused(L.EINVAL, "weights", lambda: D.ctx.bpd(b, delta, np.nan))
        refused(L.EDIM, "length(w)", lambda: D.ctx.bpd(b, delta, np.ones(N - 1)))
        refused(L.EINVAL, "rho", lambda: D.ctx.bpd(b, delta, rho=0.0))
        refused(L.EINVAL, "rho", lambda: D.ctx.bpd(b, delta, rho=-1.0))
        refused(L.EINVAL, "tol", lambda: D.ctx.bpd(b, delta, tol=0.0))
        refused(L.EINVAL, "tol", lambda: D.ctx.bpd(b, delta, tol=float("nan")))
        refused(L.EINVAL, "check_every", lambda: D.ctx.bpd(b, delta, check_every=0))
        refused(L.EINVAL, "rho", lambda: D.ctx.bpd_reweighted(b, delta, "candes", rho=0.0))
        refused(L.EINVAL, "eps", lambda: D.ctx.bpd_reweighted(b, 0.0, "candes"))  # eps = delta = 0
        refused(L.EINVAL, "scheme", lambda: D.ctx.bpd_reweighted(b, delta, 7, eps=1e-2))
    finally:
        D.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        for fn in (lambda: S.ctx.bpd(b, delta), lambda: S.ctx.bpd_reweighted(b, delta, "candes")):
            with pytest.raises(cs.CsmpError) as e:
                fn()
            assert e.value.code == L.ESTATE
    finally:
        S.close()


def test_maxiter_reached_is_no_error(cs):
    A, _, b, _, delta = tw.case_data("vertex_32x64")
    x, info = cs.bpd(A, b, delta, rho=tw.RHO, maxiter=32, return_info=True)
    assert info["iterations"] == 32 and not info["converged"] and info["factored"]
    zt, _ = tw.bpd(A, b, delta, rho=tw.RHO, maxiter=32)
    assert np.max(np.abs(x.to_dense() - zt)) <= tw.RTOL * np.max(np.abs(zt))
    x0, info0 = cs.bpd(A, b, delta, rho=tw.RHO, maxiter=0, return_info=True)
    assert x0.nnz == 0 and info0["iterations"] == 0 and not info0["converged"] and info0["resnorm"] == pytest.approx(np.linalg.norm(b), rel=1e-14)


# ------------------------------------------------------------------------------------------ device pointers
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["b_f32", "b_f64"])
def test_device_pointers(cs, dtype):
    import torch
    A, _, b, w, delta = tw.case_data("weighted_100x257")
    N = A.shape[1]
    D = cs.Dictionary(A)
    try:
        bh = b.astype(dtype)
        D.ctx.bpd(bh, delta, w, maxiter=0)  # (the call that factorises)
        want, winfo = D.ctx.bpd(bh, delta, w, maxiter=256, **KW)
        bt_ = torch.from_numpy(bh).cuda()
        xt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        info = D.ctx.bpd_device(bt_, delta, w, xt, maxiter=256, **KW)
        assert np.array_equal(xt.cpu().numpy(), want) and info == winfo and not info["factored"]
        for scheme in ("candes", "ard"):
            rw = D.ctx.bpd_reweighted(bh, delta, scheme, outer_maxiter=2, min_decrease=0.0, maxiter=256, return_weights=True, **KW)
            wt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
            rn, done = D.ctx.bpd_reweighted_device(bt_, delta, scheme, xt, wt, outer_maxiter=2, min_decrease=0.0, maxiter=256, **KW)
            assert np.array_equal(xt.cpu().numpy(), rw[0]) and rn == rw[1] and done == rw[2] == 2 and np.array_equal(wt.cpu().numpy(), rw[3])
            rn2, _ = D.ctx.bpd_reweighted_device(bt_, delta, scheme, xt, None, outer_maxiter=2, min_decrease=0.0, maxiter=256, **KW)
            assert rn2 == rn and np.array_equal(xt.cpu().numpy(), rw[0])
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_bp.py's pattern: every device allocation of a bpd call fails in turn with CSMP_ENOMEM, the same context then
    returns the clean context's bits, and the library holds what it held before."""
    L = cs._lib
    A, _, b, _, delta = tw.case_data("recover_32x48")
    gc.collect()
    base = L.live_resources()

    def solve(ctx):
        x, info = ctx.bpd(b, delta, **KW)
        return x, np.array([info["iterations"], info["converged"], info["resnorm"]])

    def reweighted(ctx):
        return ctx.bpd_reweighted(b, delta, "ard", ard_iter=2, outer_maxiter=2, min_decrease=0.0, return_weights=True, **KW)

    # bpd: the 8 buffers of the iterates, the 8 of the factor and the M-vectors, A A' and the partials of k_rowgram (the temporaries of the
    # factorisation; after the solver slot's); reweighted: csmp_bp_reweighted's 19 besides
    for call, least in ((solve, 18), (reweighted, 18 + 19)):
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
        d.ctx.bpd(b, delta, **KW)
        d.close()
    gc.collect()
    assert L.live_resources() == base
