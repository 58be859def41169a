"""numpy Float64 restatement of csmp_bpd / csmp_bpd_reweighted, straight from the recurrences of include/csmp.h, and the seeded cases the
CPU and the GPU tests share.  A plain helper module in the manner of tests/bp_twin.py: the parity yardstick of tests/test_bpd_static.py
and tests/test_gpu_bpd.py.  Nothing here reads the reference.

    bpd         min Σ w_j |x_j|  subject to  ‖A x − b‖₂ ≤ δ,  by graph-form ADMM: block one is (x, s) on the subspace s = A x, block two
                (z, v) with Σ w|z| + indicator(‖v − b‖ ≤ δ); scaled duals u (x = z) and λ (s = v), penalty ρ, K = I + A Aᵀ = L Lᵀ.
                p = A z and q = A u are carried as M-vectors:
                    e  = v − λ − p + q;   y = K⁻¹ e;   c = Aᵀ y;   t = z + c
                    z⁺ = shrink(t, w/ρ);   u⁺ = t − z⁺;   r = b − A z⁺
                    p⁺ = b − r;   q⁺ = p + (e − y) − p⁺                          (A Aᵀ y = (K − I) y = e − y)
                    h  = v − y − b;   v⁺ = b + h · (δ / ‖h‖ where ‖h‖ > δ, else 1);   λ⁺ = v − y − v⁺
                every check_every iterations: stop when √(‖u⁺−u‖² + ‖λ⁺−λ‖²) < tol and ρ √(‖z⁺−z‖² + ‖v⁺−v‖²) < tol.  The result is z.
    outer loop  z = solve(1);  for i = 2 … maxiter:  w from z;  zs = solve(w), warm-started from z, u, p, q, v, λ;
                ‖zs − z‖ < min_decrease: return zs;  z = zs
"""
import functools

import numpy as np

import bp_twin as bt
import reweight_twin as rt

RTOL = 1e-6
TWIN_TOL = 1e-9
CHECK_EVERY = 32
RHO = 100.0


class State:
    """the iterates a warm start carries over"""

    def __init__(self, M, N):
        self.z, self.u = np.zeros(N), np.zeros(N)
        self.p, self.q, self.v, self.lam = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)


def factor(A):
    A = np.asarray(A, dtype=np.float64)
    return A, np.linalg.cholesky(np.eye(A.shape[0]) + A @ A.T)


def solve(A, L, b, delta, w, st, rho, maxiter=16384, tol=1e-8, check_every=32):
    """iterates st in place; returns (iterations, converged)"""
    thr = w / rho
    for it in range(1, maxiter + 1):
        e = st.v - st.lam - st.p + st.q
        y = np.linalg.solve(L.T, np.linalg.solve(L, e))
        t = st.z + A.T @ y
        zn = bt.shrink(t, thr)
        un = t - zn
        r = b - A @ zn
        pn = b - r
        qn = st.p + (e - y) - pn
        h = st.v - y - b
        nh = np.linalg.norm(h)
        vn = b + h * (delta / nh if nh > delta else 1.0)
        ln = st.v - y - vn
        prim = np.sqrt(np.sum((un - st.u) ** 2) + np.sum((ln - st.lam) ** 2))
        dual = rho * np.sqrt(np.sum((zn - st.z) ** 2) + np.sum((vn - st.v) ** 2))
        st.z, st.u, st.p, st.q, st.v, st.lam = zn, un, pn, qn, vn, ln
        if it % check_every == 0 and prim < tol and dual < tol:
            return it, True
    return maxiter, False


def _weights(w, N):
    return np.ones(N) if w is None else np.broadcast_to(np.asarray(w, dtype=np.float64), (N,))


def bpd(A, b, delta, w=None, rho=RHO, maxiter=16384, tol=1e-8, check_every=32):
    """(z, info)"""
    A, L = factor(A)
    b = np.asarray(b, dtype=np.float64)
    st = State(*A.shape)
    it, ok = solve(A, L, b, delta, _weights(w, A.shape[1]), st, rho, maxiter, tol, check_every)
    return st.z + 0.0, {"iterations": it, "converged": ok, "resnorm": float(np.linalg.norm(b - A @ st.z))}


def bpd_reweighted(A, b, delta, scheme, eps=None, ard_iter=8, outer_maxiter=8, min_decrease=1e-4, rho=RHO, maxiter=16384, tol=1e-8,
                   check_every=32, return_iterations=False):
    """(z, the last weights, solves done[, the iterations of every solve])"""
    A, L = factor(A)
    b = np.asarray(b, dtype=np.float64)
    M, N = A.shape
    if eps is None:
        eps = delta if scheme == "candes" else delta ** 2
    w = np.ones(N)
    st = State(M, N)
    its = [solve(A, L, b, delta, w, st, rho, maxiter, tol, check_every)[0]]
    done = 1
    for i in range(2, outer_maxiter + 1):
        prev = st.z.copy()
        w = rt.candes_weights(prev, eps) if scheme == "candes" else rt.ard_support(A, prev, w, eps, ard_iter)
        its.append(solve(A, L, b, delta, w, st, rho, maxiter, tol, check_every)[0])
        done = i
        if np.linalg.norm(st.z - prev) < min_decrease:
            break
    return (st.z + 0.0, w, done) + ((its,) if return_iterations else ())


def certificate(A, b, delta, w, z):
    """the optimality conditions of min Σ w|x| s.t. ‖A x − b‖ ≤ δ at z (complete for δ > 0 and an active constraint): with r = b − A z,
    g = Aᵀ r and μ the median of |g_j| / w_j over the support, returns (|‖r‖ − δ| / δ, max over the support of |g_j − μ w_j sign z_j| / μ,
    max off the support of |g_j| / (μ w_j))"""
    A = np.asarray(A, dtype=np.float64)
    w = _weights(w, A.shape[1])
    r = b - A @ z
    g = A.T @ r
    on = z != 0
    mu = float(np.median(np.abs(g[on]) / w[on]))
    return (abs(float(np.linalg.norm(r)) - delta) / delta, float(np.max(np.abs(g[on] - mu * w[on] * np.sign(z[on])))) / mu,
            float(np.max(np.abs(g[~on]) / (mu * w[~on]))) if np.any(~on) else 0.0)


# The cases the CPU (twin against the certificate) and the GPU (device against the twin) tests share.  The first four are tests/bp_twin.py's
# with noise on b: default_rng(7).standard_normal(M) scaled to the norm δ = 1e-2 √M.  Twin iterations at tol = 1e-9, check_every = 32,
# ρ = 100 as found when the cases were chosen: see ITERATIONS below (the static test prints them).
#   tall_48x32     M > N (bp refuses it): unit-norm Gaussian columns, two planted atoms, δ = ‖noise‖ = 1e-2 √48
#   zero           recover_32x48's data with δ = 1.5 ‖b‖: the answer is z = 0 exactly
#   ragged_257x300 the M-vector stage over more than one 256-thread workgroup
NOISY = ("recover_32x48", "weighted_100x257", "vertex_32x64", "wide_130x1000")
CASES = NOISY + ("tall_48x32", "zero", "ragged_257x300")
STATIC_CASES = ("recover_32x48", "weighted_100x257", "vertex_32x64", "tall_48x32")


def _noise(M):
    n = np.random.default_rng(7).standard_normal(M)
    delta = 1e-2 * np.sqrt(M)
    return n * (delta / np.linalg.norm(n)), float(delta)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(A, x0, b, w, δ)"""
    if name in NOISY:
        A, x, b, w = bt.case_data(name)
    elif name == "tall_48x32":
        A, x, b = bt.data(48, 32, 2, 5)
        w = None
    elif name == "ragged_257x300":
        A, x, b = bt.data(257, 300, 12, 3)
        w = None
    elif name == "zero":
        A, x, b, w = bt.case_data("recover_32x48")
        return A, x, b, w, 1.5 * float(np.linalg.norm(b))
    else:
        raise KeyError(name)
    n, delta = _noise(A.shape[0])
    return A, x, b + n, w, delta


@functools.lru_cache(maxsize=None)
def case_twin(name):
    A, _, b, w, delta = case_data(name)
    return bpd(A, b, delta, w, rho=RHO, tol=TWIN_TOL, check_every=CHECK_EVERY)


@functools.lru_cache(maxsize=None)
def case_reweighted(name, scheme, outer_maxiter, min_decrease):
    A, _, b, _, delta = case_data(name)
    return bpd_reweighted(A, b, delta, scheme, outer_maxiter=outer_maxiter, min_decrease=min_decrease, rho=RHO, tol=TWIN_TOL,
                          check_every=CHECK_EVERY, return_iterations=True)
