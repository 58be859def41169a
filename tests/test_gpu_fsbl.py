"""GPU tests of the greedy forms of sparse Bayesian learning on the device: the N-pass and the pick alone (csmp_fsbl_score), the rank-one
step alone (csmp_fsbl_sqc), csmp_fsbl and csmp_rmps against the numpy twin (tests/fsbl_twin.py), the FSBL functor, warm starts, the
refusals, device pointers, the other solvers' kept state, and allocation failures."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as bt  # noqa: E402
import fsbl_twin as tw  # noqa: E402
import ista_twin as it_tw  # noqa: E402
import sbl_twin as st  # noqa: E402

pytestmark = pytest.mark.gpu

S2 = tw.SIGMA ** 2
MODES = {"all": tw.ALL, "add": tw.ADD, "rmp_delete": tw.RMP_DEL, "update": tw.UPD}


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ------------------------------------------------------------------------------------------ k_fsbl_score, k_fsbl_pick
def _state(N, seed):
    """(α, S, Q) with a quarter each of inactive-relevant, inactive-irrelevant, active-relevant and active-irrelevant atoms, in random
    order, and a zero column.  Every value is well conditioned, so that 1e-12 relative is a statement about the kernel and not about the
    last bit of a logarithm: with Q² = ρ S an inactive atom has δ_add = ρ − 1 − log ρ, ρ in 3 .. 50 (0.1 .. 0.7 where irrelevant); an
    active one has S = θ α, θ in 0.2 .. 0.8, and Q² = ρ S (1 − θ) -- relevant for ρ > 1, where ρ is set so that α*/α = κ lies in 3 .. 30
    or 1/30 .. 1/3 (δ_upd vanishes with cancellation at κ = 1), irrelevant for ρ in 0.1 .. 0.6 (δ_del = −ρ θ − log(1 − θ) > 0)."""
    rng = np.random.default_rng(seed)
    kind = rng.permutation(np.arange(N) % 4)
    S = 10.0 ** rng.uniform(2.0, 4.0, N)
    alpha = np.full(N, np.inf)
    theta = rng.uniform(0.2, 0.8, N)
    kappa = np.where(rng.random(N) < 0.5, rng.uniform(3.0, 30.0, N), 1.0 / rng.uniform(3.0, 30.0, N))
    act = kind >= 2
    alpha[act] = S[act] / theta[act]
    rho = np.select([kind == 0, kind == 1, kind == 2], [rng.uniform(3.0, 50.0, N), rng.uniform(0.1, 0.7, N), 1.0 + theta / ((1.0 - theta) * kappa)],
                    rng.uniform(0.1, 0.6, N))
    Q = np.sqrt(rho * S * np.where(act, 1.0 - theta, 1.0)) * rng.choice(np.array([-1.0, 1.0]), N)
    z = int(rng.integers(N))
    alpha[z], S[z], Q[z] = np.inf, 0.0, 0.0
    return alpha, S, Q, kind, z


@pytest.mark.parametrize("N", [32, 257, 300, 1000])
def test_score_and_pick(cs, N):
    """every mode: the values to 1e-12 relative, the pick exactly; a zero column has the value 0 and is never picked; of equal bests the
    lowest index wins"""
    A, _, _ = bt.data(16, N, 2, 5, np.float64)
    D = cs.Dictionary(A)
    try:
        for seed in (1, 2):
            alpha, S, Q, kind, z = _state(N, 100 * N + seed)
            for mode, m in MODES.items():
                a, s, q = alpha.copy(), S.copy(), Q.copy()
                vt = tw.values(m, a, s, q)
                best = int(np.argmin(vt) if m == tw.RMP_DEL else np.argmax(vt))
                if seed == 2:  # ties: the best atom's state copied to a later atom of its kind -- and to an earlier one where there is one
                    same = [j for j in np.flatnonzero(kind == kind[best]) if j != best and j != z]
                    for j in ([min(same)] if min(same) < best else []) + [max(same)]:
                        a[j], s[j], q[j] = a[best], s[best], q[best]
                    vt = tw.values(m, a, s, q)
                want = int(np.argmin(vt) if m == tw.RMP_DEL else np.argmax(vt))
                if seed == 2:
                    assert np.count_nonzero(vt == vt[want]) >= 2 and want == int(np.flatnonzero(vt == vt[want])[0])
                v, i, val, action = D.ctx.fsbl_score(a, s, q, mode)
                fin = np.isfinite(vt)
                assert np.array_equal(np.isfinite(v), fin) and np.all(v[~fin] == np.inf)
                err = float(np.max(np.abs(v[fin] - vt[fin]) / np.where(vt[fin] != 0, np.abs(vt[fin]), 1.0)))
                print(f"N = {N} seed {seed} {mode}: max relative error of a value {err:.3e}, pick {i} (twin {want}), action {action}")
                assert np.all((vt[fin] == 0) == (v[fin] == 0))
                assert err <= 1e-12
                assert i == want and val == v[i] and v[z] == (np.inf if m == tw.RMP_DEL else 0.0) and i != z
                sq = tw.sq(a, s, q)
                active, relevant = bool(sq[2][want]), bool(sq[3][want])
                if m == tw.RMP_DEL:
                    assert action == (tw.ACT_DEL if vt[want] < 1 else 0)
                else:
                    assert vt[want] > 0
                    assert action == (tw.ACT_ADD if not active else tw.ACT_UPD if relevant else tw.ACT_DEL)
                v2, i2, val2, action2 = D.ctx.fsbl_score(a, s, q, mode)  # the same bits on a second run
                assert np.array_equal(v, v2) and (i, val, action) == (i2, val2, action2)
        # nothing to pick: all atoms inactive and irrelevant -- the first index, the value 0, no action
        S = np.full(N, 1e3)
        v, i, val, action = D.ctx.fsbl_score(np.full(N, np.inf), S, np.sqrt(0.5 * S), "all")
        assert np.all(v == 0) and (i, val, action) == (0, 0.0, 0)
        v, i, val, action = D.ctx.fsbl_score(np.full(N, np.inf), S, np.sqrt(0.5 * S), "rmp_delete")
        assert np.all(v == np.inf) and val == np.inf and action == 0
        with pytest.raises(cs.CsmpError) as e:  # a value that is not finite is an error, not a pick
            D.ctx.fsbl_score(np.r_[2e3, np.full(N - 1, np.inf)], S, np.r_[np.nan, np.sqrt(0.5 * S[1:])], "all")  # δ_del of atom 0 is NaN
        assert e.value.code == cs._lib.EINVAL and "not finite" in str(e.value)
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ the rank-one step
# M = 32: under one wave's 64 rows; 100, 130: M % 64 != 0; 257: M > 256, odd (C⁻¹ has a padding row); 48 x 32: M > N
SQC_SHAPES = [(32, 48), (100, 257), (130, 300), (257, 300), (48, 32)]


@pytest.mark.parametrize("scalar", [0, 1], ids=["vec", "scalar"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SQC_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rank_one_step(cs, shape, dtype, scalar):
    """one add, one delete and one re-estimate from a state with three active atoms: C⁻¹, S and Q to 1e-10 of the largest entry, C⁻¹
    exactly symmetric, the scalar-load instantiation of k_fsbl_col with the bits of the 16-byte one"""
    M, N = shape
    A, _, b = bt.data(M, N, 3, 17, dtype)
    A64 = np.asarray(A, np.float64)
    _, info = tw.fsbl(A64, b, S2, maxiter=3)
    P = info["state"]
    assert len(info["history"]) == 3
    on = np.flatnonzero(np.isfinite(P.alpha))
    off = np.flatnonzero(~np.isfinite(P.alpha))
    steps = (("add", int(off[len(off) // 2]), 0.7), ("delete", int(on[0]), -1.0 / P.alpha[on[0]]),
             ("re-estimate", int(on[-1]), 1.0 / (3.0 * P.alpha[on[-1]]) - 1.0 / P.alpha[on[-1]]))
    D = cs.Dictionary(A)
    try:
        D.ctx.tune("fsbl_scalar", scalar)
        for what, i, gamma in steps:
            T = tw.State(A64, b, S2)
            T.Ci, T.S, T.Q = P.Ci.copy(), P.S.copy(), P.Q.copy()
            T.sqc(i, gamma)
            Ci, S, Q = D.ctx.fsbl_sqc(P.Ci, P.S, P.Q, i, gamma)
            eC, eS, eQ = _rel(Ci, T.Ci), _rel(S, T.S), _rel(Q, T.Q)
            print(f"{M}x{N} {np.dtype(dtype).name} {what} of atom {i}: C⁻¹ {eC:.3e}, S {eS:.3e}, Q {eQ:.3e}")
            assert max(eC, eS, eQ) <= 1e-10
            assert np.array_equal(Ci, Ci.T)
            Ci2, S2_, Q2 = D.ctx.fsbl_sqc(P.Ci, P.S, P.Q, i, gamma)  # the same bits on a second run
            assert np.array_equal(Ci, Ci2) and np.array_equal(S, S2_) and np.array_equal(Q, Q2)
            D.ctx.tune("fsbl_scalar", 1 - scalar)
            Ci3, S3, Q3 = D.ctx.fsbl_sqc(P.Ci, P.S, P.Q, i, gamma)
            D.ctx.tune("fsbl_scalar", scalar)
            assert np.array_equal(Ci, Ci3) and np.array_equal(S, S3) and np.array_equal(Q, Q3)
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ parity, recovery
def _run(ctx, solver, y, **kw):
    return getattr(ctx, solver)(y, S2, **kw)


@pytest.mark.parametrize("name,solver", tw.RUNS)
def test_parity_with_the_twin(cs, name, solver):
    """the history of (action, index) is the twin's -- the last step excepted where its value is below min_increase: such a re-estimate
    may name another atom --, the same active set, x and the finite α within 1e-6, iterations and converged equal"""
    A, x0, b, y = tw.case_data(name)
    xt, it = tw.case_twin(name, solver)
    D = cs.Dictionary(A)
    try:
        x, info = _run(D.ctx, solver, y)
    finally:
        D.close()
    applied = [r["value"] for r in it["records"] if r["action"]]
    n = len(applied) - (1 if applied and applied[-1] < tw.MIN_INCREASE else 0)
    fin = np.isfinite(it["alpha"])
    ex = float(np.max(np.abs(x - xt)) / np.max(np.abs(xt)))
    ea = float(np.max(np.abs(info["alpha"][fin] - it["alpha"][fin]) / it["alpha"][fin])) if np.array_equal(np.isfinite(info["alpha"]), fin) else np.inf
    print(f"{name} {solver}: {len(info['history'])} steps (twin {len(it['history'])}), {info['iterations']} iterations (twin {it['iterations']}), "
          f"max|x − twin| / max|x| = {ex:.3e}, max rel |α − twin| = {ea:.3e}")
    assert len(info["history"]) == len(it["history"]) and info["history"][:n] == it["history"][:n]
    assert info["iterations"] == it["iterations"] and info["converged"] == it["converged"]
    assert np.array_equal(np.isfinite(info["alpha"]), fin) and np.array_equal(x != 0, fin)
    assert ex <= tw.RTOL and ea <= tw.RTOL
    if name in st.CASES:
        assert st.recovers(A, x, x0, b)


def test_recovery_of_the_reference_test(cs):
    """test/sbl.jl:20-27: 32 x 48, k = 3, σ = 1e-2, y = perturb(b, σ / 2): the entries above σ are the planted support, A x ≈ b to σ"""
    for seed in (0, 1, 2):
        A, x0, b = cs.sparse_data(32, 48, 3, rng=seed)
        y = cs.perturb(b, tw.SIGMA / 2, rng=100 + seed)
        for fn in (cs.fsbl, cs.rmps):
            x = fn(A, y, S2)
            print(f"seed {seed} {fn.__name__}: support {np.flatnonzero(np.abs(x) > tw.SIGMA)}, ‖A x − b‖ = {np.linalg.norm(A @ x - b):.3e}")
            assert np.array_equal(np.flatnonzero(np.abs(x) > tw.SIGMA), x0.nzind)
            assert np.linalg.norm(A @ x - b) <= tw.SIGMA


# ------------------------------------------------------------------------------------------ caps, history, repeatability, step form
def test_reaching_a_cap_is_no_error(cs):
    A, _, _, y = tw.case_data("32x48k8s19_f64")
    D = cs.Dictionary(A)
    try:
        x, info = D.ctx.fsbl(y, S2, maxiter=5)
        xt, it = tw.fsbl(A, y, S2, maxiter=5)
        assert info["iterations"] == 5 and not info["converged"] and info["history"] == it["history"]
        assert _rel(x, xt) <= tw.RTOL
        for kw in (dict(maxiter=1), dict(maxiter=2, maxiter_acquisition=3), dict(maxiter=3, maxiter_deletion=1)):
            x, info = D.ctx.rmps(y, S2, **kw)
            xt, it = tw.rmps(A, y, S2, **kw)
            assert info["converged"] == it["converged"] == ("maxiter_deletion" in kw)  # (the third run ends on its own: alpha stops changing)
            assert info["history"] == it["history"] and info["iterations"] == it["iterations"] == len(it["history"])
            assert _rel(x, xt) <= tw.RTOL
    finally:
        D.close()


def test_history_cap_smaller_than_the_run(cs):
    A, _, _, y = tw.case_data("100x257k20s23_f32")
    D = cs.Dictionary(A)
    try:
        for solver in ("fsbl", "rmps"):
            x, full = _run(D.ctx, solver, y)
            assert len(full["history"]) > 7
            for cap in (0, 7):
                xc, part = _run(D.ctx, solver, y, history_cap=cap)
                assert part["history"] == full["history"][:cap] and part["iterations"] == full["iterations"] and np.array_equal(xc, x)
    finally:
        D.close()


def test_two_runs_give_the_same_bits(cs):
    A, _, _, y = tw.case_data("130x1000_f32")
    for solver in ("fsbl", "rmps"):
        D = cs.Dictionary(A)
        try:
            a = _run(D.ctx, solver, y)
            b = _run(D.ctx, solver, y)
        finally:
            D.close()
        D = cs.Dictionary(A)
        try:
            c = _run(D.ctx, solver, y)
        finally:
            D.close()
        for u in (b, c):
            assert np.array_equal(a[0], u[0]) and np.array_equal(a[1]["alpha"], u[1]["alpha"])
            assert {k: v for k, v in a[1].items() if k != "alpha"} == {k: v for k, v in u[1].items() if k != "alpha"}


@pytest.mark.parametrize("name,t,tol", [("100x257_f32", 12, 1e-9), ("32x48k8s19_f32", 24, tw.RTOL)])
def test_step_form(cs, name, t, tol):
    """the FSBL functor stepped t times: the history of fsbl(maxiter = t), x to 1e-9.  Every call replays the active set from I/σ², so
    its state carries none of the run's rounding history: on the second case, whose first 24 passes delete atoms -- the twin's recurrences
    are 7e-9 off the from-scratch form there (tests/fsbl_twin.py) -- the histories are compared, and x by the parity contract."""
    A, _, _, y = tw.case_data(name)
    D = cs.Dictionary(A)
    P = cs.FSBL(D, y, S2)
    try:
        want, winfo = cs.fsbl(D, y, S2, maxiter=t, return_info=True)
        assert any(a == tw.ACT_DEL for a, _ in winfo["history"]) == (tol != 1e-9)
        for _ in range(t):
            x = P()
        print(f"{name}: max|x − fsbl(maxiter = {t})| / max|x| = {_rel(x, want):.3e}")
        assert P.iterations == t and P.history == winfo["history"]
        assert _rel(x, want) <= tol and np.array_equal(P.x, x)
        assert np.array_equal(np.isfinite(P.alpha.cpu().numpy()), np.isfinite(winfo["alpha"]))
        out = np.zeros(A.shape[1])
        assert P.update_(out) is out  # update!(P, x) fills x
    finally:
        P.close()
        D.close()


@pytest.mark.parametrize("name,t", [("32x48k8s19_f64", 21), ("100x257k20s23_f32", 30)])
def test_warm_start_from_a_twin_alpha(cs, name, t):
    A, _, _, y = tw.case_data(name)
    A64 = np.asarray(A, np.float64)
    xt, it = tw.case_twin(name, "fsbl")
    _, head = tw.fsbl(A64, y, S2, maxiter=t)
    D = cs.Dictionary(A)
    try:
        x, info = D.ctx.fsbl(y, S2, alpha=head["alpha"])
        assert head["history"] + info["history"] == it["history"] and t + info["iterations"] == it["iterations"] and info["converged"]
        assert _rel(x, xt) <= tw.RTOL
        xr, ir = D.ctx.rmps(y, S2, alpha=head["alpha"])
        xrt, irt = tw.rmps(A64, y, S2, alpha=head["alpha"])
        assert ir["history"] == irt["history"] and _rel(xr, xrt) <= tw.RTOL
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ device pointers
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["b_f32", "b_f64"])
def test_device_pointers(cs, dtype):
    import torch
    A, _, _, y = tw.case_data("100x257k20s23_f32")
    N = A.shape[1]
    D = cs.Dictionary(A)
    try:
        yh = y.astype(dtype)
        yt = torch.from_numpy(yh).cuda()
        for solver in ("fsbl", "rmps"):
            want, winfo = _run(D.ctx, solver, yh)
            xt = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
            at = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            info = getattr(D.ctx, solver + "_device")(yt, S2, xt, None, at, history_cap=len(winfo["history"]))
            assert info == {k: v for k, v in winfo.items() if k != "alpha"}
            assert np.array_equal(xt.cpu().numpy(), want) and np.array_equal(at.cpu().numpy(), winfo["alpha"])
            info = getattr(D.ctx, solver + "_device")(yt, S2, xt)  # alpha_out and the history are optional
            assert info["iterations"] == winfo["iterations"] and info["history"] == [] and np.array_equal(xt.cpu().numpy(), want)
        # alpha_in in device memory, alpha_out in its place
        _, head = D.ctx.fsbl(yh, S2, maxiter=12)
        want, winfo = D.ctx.fsbl(yh, S2, alpha=head["alpha"])
        at = torch.from_numpy(head["alpha"]).cuda()
        info = D.ctx.fsbl_device(yt, S2, xt, at, at, history_cap=512)
        assert info["history"] == winfo["history"] and np.array_equal(xt.cpu().numpy(), want) and np.array_equal(at.cpu().numpy(), winfo["alpha"])
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(cs):
    import torch
    L = cs._lib
    A, _, _, y = tw.case_data("32x48_f64")
    M, N = A.shape
    D = cs.Dictionary(A)
    want = D.ctx.fsbl(y, S2)[0]

    def refused(code, text, fn):
        with pytest.raises(cs.CsmpError) as e:
            fn()
        assert e.value.code == code and text in str(e.value), (code, str(e.value))
        assert np.array_equal(D.ctx.fsbl(y, S2)[0], want)  # the context still solves

    try:
        for solver, caps in (("fsbl", ("maxiter",)), ("rmps", ("maxiter", "maxiter_acquisition", "maxiter_deletion"))):
            run = getattr(D.ctx, solver)
            for s2 in (0.0, -1e-4, float("inf"), float("nan")):
                refused(L.EINVAL, "sigma2", lambda: run(y, s2))
            refused(L.EINVAL, "min_increase", lambda: run(y, S2, min_increase=-1.0))
            refused(L.EINVAL, "min_increase", lambda: run(y, S2, min_increase=float("nan")))
            for c in caps:
                refused(L.EINVAL, c, lambda: run(y, S2, **{c: 0}))
            for bad in (0.0, -1.0, -np.inf, np.nan):
                a = np.full(N, np.inf)
                a[7] = bad
                refused(L.EINVAL, "alpha", lambda: run(y, S2, alpha=a))
                at, bt_, xt = torch.from_numpy(a).cuda(), torch.from_numpy(y).cuda(), torch.zeros(N, dtype=torch.float64, device="cuda")
                refused(L.EINVAL, "alpha", lambda: getattr(D.ctx, solver + "_device")(bt_, S2, xt, at))
            refused(L.EDIM, "length(alpha)", lambda: run(y, S2, alpha=np.full(N - 1, np.inf)))
            refused(L.EDIM, "length(b)", lambda: run(y[:-1], S2))
        x = np.zeros(N)
        it, fl = L.i64(0), L.C.c_int(0)
        head = (L.C.c_double(S2), L.i64(4), L.C.c_double(1e-6), None)
        tail = (L.HOST, None, L.i64(0), L.C.byref(it), L.C.byref(fl))
        refused(L.EINVAL, "bad arguments", lambda: D.ctx.call("csmp_fsbl", None, L.F64, *head, L.ptr(x), None, *tail))
        refused(L.EINVAL, "bad arguments", lambda: D.ctx.call("csmp_fsbl", L.ptr(y), L.F64, *head, None, None, *tail))
        refused(L.EINVAL, "b_dtype", lambda: D.ctx.call("csmp_fsbl", L.ptr(y), 7, *head, L.ptr(x), None, *tail))
        refused(L.EINVAL, "loc", lambda: D.ctx.call("csmp_fsbl", L.ptr(y), L.F64, *head, L.ptr(x), None, 7, *tail[1:]))
        D.ctx.call("csmp_fsbl", L.ptr(y), L.F64, *head, L.ptr(x), None, L.HOST, None, L.i64(0), None, None)  # everything optional may be NULL
        assert np.array_equal(x, D.ctx.fsbl(y, S2, maxiter=4)[0])
        for fn in (cs.fsbl, cs.rmps, cs.FSBL):
            with pytest.raises(NotImplementedError):
                fn(D, y, S2 * np.eye(M))
        with pytest.raises(NotImplementedError):
            cs.rmps(D, y, True)
        refused(L.EINVAL, "column of A", lambda: D.ctx.fsbl_sqc(np.eye(M), np.ones(N), np.ones(N), N, 1.0))
        refused(L.EINVAL, "gamma", lambda: D.ctx.fsbl_sqc(np.eye(M), np.ones(N), np.ones(N), 0, 0.0))
        refused(L.EINVAL, "mode", lambda: D.ctx.call("csmp_fsbl_score", L.ptr(x), L.ptr(x), L.ptr(x), 9, L.ptr(x), None, None, None))
    finally:
        D.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        for fn in (lambda: S.ctx.fsbl(y, S2), lambda: S.ctx.rmps(y, S2), lambda: S.ctx.fsbl_score(np.ones(N), np.ones(N), np.ones(N), "all"),
                   lambda: S.ctx.fsbl_sqc(np.eye(M), np.ones(N), np.ones(N), 0, 1.0)):
            with pytest.raises(cs.CsmpError) as e:
                fn()
            assert e.value.code == L.ESTATE
    finally:
        S.close()
    c = cs.Context(0)
    try:
        c.M, c.N = M, N
        for fn in (c.fsbl, c.rmps):
            with pytest.raises(cs.CsmpError) as e:
                fn(y, S2)
            assert e.value.code == L.ESTATE and "no dictionary" in str(e.value)
        with pytest.raises(cs.CsmpError) as e:
            c.bench_fsbl()
        assert e.value.code == L.ESTATE
    finally:
        c.close()


# ------------------------------------------------------------------------------------------ the other solvers
def test_other_solvers_are_undisturbed(cs):
    A, _, b, alpha, _ = it_tw.case_data("256x1024_f32")
    delta = 1e-2 * float(np.linalg.norm(b))
    D = cs.Dictionary(A)
    try:
        z1, i1 = D.ctx.bp(b, maxiter=128)
        d1, j1 = D.ctx.bpd(b, delta, maxiter=128)
        a1 = D.ctx.ista(b, 2e-2, maxiter=64, stepsize=alpha)
        s1 = D.ctx.sbl(b, S2, maxiter=2, return_gamma=True)
        o1 = D.ctx.omp(b, 8, 0.0)
        assert i1["factored"] and j1["factored"]
        f1 = D.ctx.fsbl(b, S2, maxiter=12)
        r1 = D.ctx.rmps(b, S2, maxiter=1, maxiter_acquisition=6)
        z2, i2 = D.ctx.bp(b, maxiter=128)
        d2, j2 = D.ctx.bpd(b, delta, maxiter=128)
        a2 = D.ctx.ista(b, 2e-2, maxiter=64, stepsize=alpha)
        s2 = D.ctx.sbl(b, S2, maxiter=2, return_gamma=True)
        o2 = D.ctx.omp(b, 8, 0.0)
        f2 = D.ctx.fsbl(b, S2, maxiter=12)
        assert not i2["factored"] and not j2["factored"]  # the kept factors are still the kept factors
        assert np.array_equal(z1, z2) and i1["iterations"] == i2["iterations"] and i1["resnorm"] == i2["resnorm"]
        assert np.array_equal(d1, d2) and j1["iterations"] == j2["iterations"] and j1["resnorm"] == j2["resnorm"]
        assert np.array_equal(a1[0], a2[0]) and a1[1] == a2[1]
        assert np.array_equal(s1[0], s2[0]) and s1[1] == s2[1] and np.array_equal(s1[2], s2[2])
        assert all(np.array_equal(u, v) for u, v in zip(o1, o2))
        assert np.array_equal(f1[0], f2[0]) and f1[1]["history"] == f2[1]["history"] and len(f1[1]["history"]) == 12
        assert len(r1[1]["history"]) >= 6
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_sbl.py's pattern: every device allocation of a call fails in turn with CSMP_ENOMEM, the same context then returns
    the clean context's bits, and the library holds what it held before."""
    L = cs._lib
    A, _, _, y = tw.case_data("32x48k8s16_f64")
    M, N = A.shape
    P = tw.case_twin("32x48k8s16_f64", "fsbl")[1]["state"]
    gc.collect()
    base = L.live_resources()

    def solve(ctx):
        x, info = ctx.fsbl(y, S2)
        return x, info["alpha"], np.array(info["history"]), np.array([info["iterations"], info["converged"]])

    def solve_rmps(ctx):
        x, info = ctx.rmps(y, S2)
        return x, info["alpha"], np.array(info["history"])

    def score(ctx):
        return ctx.fsbl_score(P.alpha, P.S, P.Q, "all")[:1]

    def sqc(ctx):
        return ctx.fsbl_sqc(P.Ci, P.S, P.Q, 3, 0.5)

    # the ten buffers of FsblBuf (beside the solver slot the sweep runs on)
    for call, least in ((solve, 10), (solve_rmps, 10), (score, 10), (sqc, 10)):
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
                if call is solve:
                    assert "size(A,1)^2 doubles" in str(e)
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
        d.ctx.fsbl(y, S2)
        d.close()
    gc.collect()
    assert L.live_resources() == base
