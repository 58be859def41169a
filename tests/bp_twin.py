"""numpy Float64 restatement of csmp_bp / csmp_bp_reweighted, straight from the recurrences of include/csmp.h, and the seeded cases the
CPU and the GPU tests share.  A plain helper module: the parity yardstick of tests/test_bp_static.py and tests/test_gpu_bp.py.
Nothing here reads the reference.

    bp          min Σ w_j |x_j|  subject to  A x = b,  by ADMM on the split x = z with G = A Aᵀ, scaled dual u, penalty ρ.
                p = A z and q = A u are carried as M-vectors:
                    e  = p − q − b;   y = G⁻¹ e;   c = Aᵀ y;   t = z − c
                    z⁺ = shrink(t, w/ρ);   u⁺ = t − z⁺
                    r  = b − A z⁺;   p⁺ = b − r;   q⁺ = p − G y − p⁺
                every check_every iterations: stop when ‖u⁺ − u‖ < tol and ρ‖z⁺ − z‖ < tol.  The result is z.
    outer loop  z = solve(1);  for i = 2 … maxiter:  w from z;  zs = solve(w), warm-started from z, u, p, q;  ‖zs − z‖ < min_decrease:
                return zs;  z = zs
"""
import functools

import numpy as np

import reweight_twin as rt

RTOL = 1e-6


def shrink(t, a):
    return np.sign(t) * np.maximum(np.abs(t) - a, 0.0)


def data(M, N, k, seed, dtype=np.float64):
    """the generator of the package's sparse_data (src/util.jl:21-31): Gaussian columns, mean shifted by 1e-6, unit norms, rounded to
    dtype once; a planted ±1 signal on k atoms; b = A x in Float64"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N))
    A -= 1e-6 * A.mean(axis=0, keepdims=True)
    A /= np.sqrt((A * A).sum(axis=0, keepdims=True))
    A = np.asfortranarray(A.astype(dtype))
    ind = np.sort(rng.choice(N, size=k, replace=False))
    val = rng.choice(np.array([-1.0, 1.0]), size=k)
    x = np.zeros(N)
    x[ind] = val
    return A, x, A.astype(np.float64) @ x


class State:
    """the iterates a warm start carries over"""

    def __init__(self, M, N):
        self.z, self.u, self.p, self.q = np.zeros(N), np.zeros(N), np.zeros(M), np.zeros(M)


def factor(A):
    A = np.asarray(A, dtype=np.float64)
    G = A @ A.T
    return A, G, np.linalg.cholesky(G)


def solve(A, G, L, b, w, st, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
    """iterates st in place; returns (iterations, converged)"""
    thr = w / rho
    for it in range(1, maxiter + 1):
        e = st.p - st.q - b
        y = np.linalg.solve(L.T, np.linalg.solve(L, e))
        t = st.z - A.T @ y
        zn = shrink(t, thr)
        un = t - zn
        r = b - A @ zn
        pn = b - r
        qn = st.p - G @ y - pn
        prim, dual = np.linalg.norm(un - st.u), rho * np.linalg.norm(zn - st.z)
        st.z, st.u, st.p, st.q = zn, un, pn, qn
        if it % check_every == 0 and prim < tol and dual < tol:
            return it, True
    return maxiter, False


def bp(A, b, w=None, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
    """(z, info)"""
    A, G, L = factor(A)
    b = np.asarray(b, dtype=np.float64)
    N = A.shape[1]
    w = np.ones(N) if w is None else np.broadcast_to(np.asarray(w, dtype=np.float64), (N,))
    st = State(*A.shape)
    it, ok = solve(A, G, L, b, w, st, rho, maxiter, tol, check_every)
    return st.z + 0.0, {"iterations": it, "converged": ok, "resnorm": float(np.linalg.norm(b - A @ st.z))}


def bp_reweighted(A, b, scheme, eps=1e-2, ard_iter=8, outer_maxiter=8, min_decrease=1e-8, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
    """(z, the last weights, solves done)"""
    A, G, L = factor(A)
    b = np.asarray(b, dtype=np.float64)
    M, N = A.shape
    w = np.ones(N)
    st = State(M, N)
    solve(A, G, L, b, w, st, rho, maxiter, tol, check_every)
    done = 1
    for i in range(2, outer_maxiter + 1):
        prev = st.z.copy()
        w = rt.candes_weights(prev, eps) if scheme == "candes" else rt.ard_support(A, prev, w, eps, ard_iter)
        solve(A, G, L, b, w, st, rho, maxiter, tol, check_every)
        done = i
        if np.linalg.norm(st.z - prev) < min_decrease:
            break
    return st.z + 0.0, w, done


def lp(A, b, w=None):
    """min Σ w_j |x_j| s.t. A x = b as a linear programme (x = x⁺ − x⁻), by HiGHS"""
    from scipy.optimize import linprog
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[1]
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    res = linprog(np.concatenate([w, w]), A_eq=np.hstack([A, -A]), b_eq=b, bounds=(0, None), method="highs")
    assert res.status == 0, res.message
    return res.x[:N] - res.x[N:]


# the cases the CPU (twin against the LP) and the GPU (device against the twin) tests share: name -> (M, N, k, seed, dtype, weighted)
# twin iterations at tol = 1e-9 (check_every = 32), nnz of the result:
#   recover_32x48      64 iterations, nnz 3 (= x0), 6e-12 from the LP
#   weighted_100x257   160 iterations, nnz 10 (= x0), 5e-12 from the LP
#   vertex_32x64       l1 does NOT recover x0 (k = 12; seeds 2, 4, 8 and 9 of 0 .. 11 do this, seed 4 is taken): the solution is a full
#                      vertex, nnz = M = 32, smallest entry 8.3e-3; 6944 iterations, 3.5e-9 from the LP
#   wide_130x1000      448 iterations, nnz 12 (= x0), 3e-10 from the LP
CASES = {
    "recover_32x48": (32, 48, 3, 0, np.float64, False),
    "weighted_100x257": (100, 257, 10, 1, np.float32, True),
    "vertex_32x64": (32, 64, 12, 4, np.float64, False),
    "wide_130x1000": (130, 1000, 12, 2, np.float32, False),
}
STATIC_CASES = ("recover_32x48", "weighted_100x257", "vertex_32x64")
TWIN_TOL = 1e-9


@functools.lru_cache(maxsize=None)
def case_data(name):
    M, N, k, seed, dtype, weighted = CASES[name]
    A, x, b = data(M, N, k, seed, dtype)
    w = np.random.default_rng(1000 + seed).uniform(0.5, 2.0, N) if weighted else None
    return A, x, b, w


@functools.lru_cache(maxsize=None)
def case_twin(name):
    A, _, b, w = case_data(name)
    return bp(A, b, w, tol=TWIN_TOL)
