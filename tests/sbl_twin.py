"""numpy Float64 restatement of csmp_sbl, straight from the recurrences of include/csmp.h, beside the reference's own form of the same
update (src/sbl.jl:26-35, restated), and the seeded cases the CPU and the GPU tests share.  A plain helper module: the parity yardstick of
tests/test_sbl_static.py and tests/test_gpu_sbl.py.  Nothing here reads the reference.

    Woodbury    C = σ² I + A Γ Aᵀ = L Lᵀ (M × M);  P = L⁻¹ A;  t = L⁻¹ b;  s_j = ‖p_j‖²;  q_j = p_jᵀ t
                x_j = γ_j q_j;   γ_j⁺ = γ_j q_j² / s_j + 1e-14        (s_j = 0: x_j = 0, γ_j⁺ = 1e-14)
    direct      B = AᵀA / σ² + Γ⁻¹ (N × N);  x = B⁻¹ Aᵀ b / σ²;  γ_j⁺ = x_j² / (1 − (B⁻¹)_jj / γ_j) + 1e-14
    loop        γ = 1;  after every update stop when ‖γ_old − γ‖₂ < min_change, at the latest after maxiter (default 128 N) updates
"""
import functools

import numpy as np

import bp_twin as bt

RTOL = 1e-6       # the project's parity contract: ‖x − x_twin‖∞ ≤ RTOL ‖x_twin‖∞, the same for γ
FLOOR = 1e-14
MIN_CHANGE = 1e-6
SIGMA = 1e-2      # test/sbl.jl:9


def _check(A, b, sigma2, maxiter, min_change, gamma):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if np.ndim(sigma2) != 0:
        raise NotImplementedError("sbl: a noise covariance matrix Σ is not served: scalar σ² only")
    if A.ndim != 2 or b.shape != (A.shape[0],):
        raise ValueError("DimensionMismatch")
    if not (sigma2 > 0 and np.isfinite(sigma2)):
        raise ValueError("σ² has to be positive and finite")
    if not min_change >= 0:
        raise ValueError("min_change has to be non-negative")
    if maxiter is not None and maxiter < 1:
        raise ValueError("maxiter has to be at least 1")
    N = A.shape[1]
    gamma = np.ones(N) if gamma is None else np.array(gamma, dtype=np.float64)
    if gamma.shape != (N,) or not np.all((gamma > 0) & np.isfinite(gamma)):
        raise ValueError("every entry of gamma has to be positive and finite")
    return A, b, float(sigma2), (128 * N if maxiter is None else int(maxiter)), gamma


def forms(A, L, b):
    """(s, q, P, t) of the N-pass: the projections of every atom on the columns of L⁻ᵀ"""
    P = np.linalg.solve(L, A)
    t = np.linalg.solve(L, b)
    return np.sum(P * P, axis=0), P.T @ t, P, t


def update_woodbury(A, b, sigma2, gamma):
    """one update in csmp_sbl's form: (x, γ⁺)"""
    C = sigma2 * np.eye(A.shape[0]) + (A * gamma) @ A.T
    s, q, _, _ = forms(A, np.linalg.cholesky(C), b)
    live = s != 0.0
    x = np.where(live, gamma * q, 0.0)
    g = np.where(live, gamma * q * q / np.where(live, s, 1.0) + FLOOR, FLOOR)
    return x, g


def update_direct(A, b, sigma2, gamma):
    """the same update as the reference writes it, on the N × N matrix: (x, γ⁺)"""
    B = A.T @ A / sigma2 + np.diag(1.0 / gamma)
    x = np.linalg.solve(B, A.T @ b / sigma2)
    d = np.diag(np.linalg.inv(B))
    return x, x * x / (1.0 - d / gamma) + FLOOR


def sbl(A, b, sigma2, maxiter=None, min_change=MIN_CHANGE, gamma=None, form="woodbury"):
    """(x of the last update, info = iterations, converged, gamma, history: ‖γ_old − γ‖ of every update)"""
    A, b, sigma2, maxiter, gamma = _check(A, b, sigma2, maxiter, min_change, gamma)
    step = update_woodbury if form == "woodbury" else update_direct
    x, hist, conv = np.zeros(A.shape[1]), [], False
    for _ in range(maxiter):
        x, g = step(A, b, sigma2, gamma)
        hist.append(float(np.linalg.norm(gamma - g)))
        gamma = g
        if hist[-1] < min_change:
            conv = True
            break
    return x, {"iterations": len(hist), "converged": conv, "gamma": gamma, "history": hist}


def recovers(A, x, x0, b0, sigma=SIGMA):
    """test/sbl.jl:16-17: the entries above σ are the planted support, and A x ≈ b to σ (isapprox with atol: the 2-norm)"""
    A = np.asarray(A, dtype=np.float64)
    return np.array_equal(np.flatnonzero(np.abs(x) > sigma), np.flatnonzero(x0)) and np.linalg.norm(A @ x - b0) <= sigma


# name -> (M, N, k, seed, dtype): sparse_data's generator (bp_twin.data), y = b + e with ‖e‖ = σ / 2 (perturb), σ² = 1e-4.
# Updates of the twin and the ‖Δγ‖ of its history nearest to min_change = 1e-6 (tests/test_sbl_static.py asserts none within 10 %), the
# same for both element types: 32x48 6, 4.3e-7; 100x257 6, 6.4e-7; 130x300 6, 3.4e-7; 257x300 5, 1.8e-7; 130x1000 7, 9.6e-6; 48x32 4, 3.6e-7
# (48x32 at seed 6 had 9.3e-7, inside the 10 %: seed 8 was taken instead).
CASES = {
    "32x48_f64": (32, 48, 3, 1, np.float64),
    "32x48_f32": (32, 48, 3, 1, np.float32),
    "100x257_f64": (100, 257, 8, 2, np.float64),
    "100x257_f32": (100, 257, 8, 2, np.float32),
    "130x300_f64": (130, 300, 10, 3, np.float64),
    "130x300_f32": (130, 300, 10, 3, np.float32),
    "257x300_f64": (257, 300, 12, 4, np.float64),
    "257x300_f32": (257, 300, 12, 4, np.float32),
    "130x1000_f64": (130, 1000, 8, 5, np.float64),
    "130x1000_f32": (130, 1000, 8, 5, np.float32),
    "48x32_f64": (48, 32, 3, 8, np.float64),
    "48x32_f32": (48, 32, 3, 8, np.float32),
}
DIRECT_CASES = ("32x48_f64", "100x257_f64", "130x300_f64", "48x32_f64")  # the cases the direct N × N form is run on


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(A, x0, b = A x0, y = b perturbed by σ / 2)"""
    M, N, k, seed, dtype = CASES[name]
    A, x0, b = bt.data(M, N, k, seed, dtype)
    e = np.random.default_rng(7000 + seed).standard_normal(M)
    return A, x0, b, b + e * (SIGMA / 2 / np.linalg.norm(e))


@functools.lru_cache(maxsize=None)
def case_twin(name, form="woodbury"):
    A, _, _, y = case_data(name)
    return sbl(A, y, SIGMA ** 2, form=form)
