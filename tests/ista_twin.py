"""numpy Float64 restatement of ista / fista, straight from the formulas of include/csmp.h (csmp_ista), and the seeded parity cases
the CPU and the GPU tests share.  A plain helper module: the parity yardstick of tests/test_ista_static.py and tests/test_gpu_ista.py.

    objective   ‖b − A x‖² + Σ w_j |x_j|
    ∇           Aᵀ(b − A y)
    x⁺          sign(u) max(|u| − w α, 0),  u = y + 2α∇,  α = stepsize
    ISTA        y = x
    FISTA       t₁ = 1,  t⁺ = (1 + √(1 + 4t²))/2,  y⁺ = x⁺ + ((t − 1)/t⁺)(x⁺ − x),  y₁ = x₀
Exactly maxiter iterations; the dictionary's values are promoted to Float64 exactly, as the library does."""
import functools

import numpy as np

RTOL = 1e-6  # the suite's tolerance: |x − x_twin| ≤ RTOL · max|x_twin| for every coordinate


def shrinkage(u, a):
    return np.sign(u) * np.maximum(np.abs(u) - a, 0.0)


def weights(lam_or_w, N):
    w = np.atleast_1d(np.asarray(lam_or_w, dtype=np.float64))
    return np.full(N, w[0]) if len(w) == 1 else w


def dense(x0, N):
    x = np.zeros(N)
    if x0 is not None:
        x[np.asarray(x0[0], dtype=np.int64)] = x0[1]
    return x


def ista(A, b, lam_or_w, x0=None, maxiter=1024, stepsize=1e-2):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    w = weights(lam_or_w, A.shape[1])
    x = dense(x0, A.shape[1])
    for _ in range(maxiter):
        g = A.T @ (b - A @ x)
        x = shrinkage(x + 2 * stepsize * g, w * stepsize)
    return x + 0.0  # (−0.0 → 0.0: an exact zero is a structural zero)


def fista(A, b, lam_or_w, x0=None, maxiter=1024, stepsize=1e-2):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    w = weights(lam_or_w, A.shape[1])
    x = dense(x0, A.shape[1])
    y, t = x.copy(), 1.0
    for _ in range(maxiter):
        g = A.T @ (b - A @ y)
        xn = shrinkage(y + 2 * stepsize * g, w * stepsize)
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        y = xn + ((t - 1.0) / tn) * (xn - x)
        x, t = xn, tn
    return x + 0.0


def objective(A, b, lam_or_w, x):
    A = np.asarray(A, dtype=np.float64)
    r = np.asarray(b, dtype=np.float64) - A @ x
    return float(r @ r + weights(lam_or_w, A.shape[1]) @ np.abs(x))


def stepsize(A):
    """0.45 / ‖A‖₂²: inside the 1/(2‖A‖₂²) that makes the iteration a descent method for this objective (its smooth part has the
    Lipschitz constant 2‖A‖₂²)"""
    return 0.45 / np.linalg.norm(np.asarray(A, dtype=np.float64), 2) ** 2


def planted(M, N, k, dtype, seed, noise=5e-3):
    """unit-norm Gaussian columns (normalised in Float64, then rounded to dtype), a planted ±1 signal on k atoms, b = A x + noise"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0)
    A = np.asfortranarray(A.astype(dtype))
    x = np.zeros(N)
    S = rng.choice(N, size=k, replace=False)
    x[S] = rng.choice([-1.0, 1.0], size=k)
    b = A.astype(np.float64) @ x + noise * rng.standard_normal(M)
    return A, x, b.astype(dtype)


# shape cases: name -> (M, N, k, dtype, seed, maxiter)
SHAPES = {
    "32x48_f64": (32, 48, 3, np.float64, 1, 1024),
    "256x1024_f32": (256, 1024, 16, np.float32, 2, 1024),
    "512x4096_f32": (512, 4096, 32, np.float32, 3, 1024),
    "short_256x3000_f64": (256, 3000, 16, np.float64, 4, 1024),    # columns of two chunks: k_sweep_short
    "ragged_1000x3000_f64": (1000, 3000, 40, np.float64, 5, 1024),
    "long_32768x96_f32": (32768, 96, 8, np.float32, 6, 32),         # a residual longer than the LDS (test_gpu_shapes.py: SWEEP_SHAPES), staged in phases
}
LAMBDAS = (1e-3, 2e-2, 0.2)
FISTA_LAMBDAS = (2e-2, 0.2)  # (λ = 1e-3 is the regime where two CPU runs of FISTA differ by more than the tolerance: DESIGN.md)


def parity_cases():
    """every (method, shape, variant) the GPU parity tests run; variant: a λ, "weights" or "warm" """
    cases = [("ista", s, lam) for s in SHAPES for lam in LAMBDAS]
    cases += [("fista", s, lam) for s in SHAPES for lam in FISTA_LAMBDAS]
    cases += [("ista", "256x1024_f32", "weights"), ("ista", "ragged_1000x3000_f64", "warm"), ("fista", "256x1024_f32", "weights"),
              ("fista", "256x1024_f32", "warm")]
    return cases


def case_id(case):
    return f"{case[0]}-{case[1]}-{case[2]}"


@functools.lru_cache(maxsize=None)
def case_data(shape):
    M, N, k, dtype, seed, maxiter = SHAPES[shape]
    A, x, b = planted(M, N, k, dtype, seed)
    return A, x, b, stepsize(A), maxiter


def case_args(case):
    """(A, b, w, x0, maxiter, stepsize) of a parity case.  "weights": a weight vector between 0 and 0.1 with every fifth weight exactly
    zero; "warm": λ = 2e-2 from a warm start of 24 entries (some on the planted support, some not)."""
    method, shape, variant = case
    A, x, b, alpha, maxiter = case_data(shape)
    N = A.shape[1]
    rng = np.random.default_rng(2000 + SHAPES[shape][4])  # (seeds chosen so that no twin result has an entry inside the band)
    w, x0 = variant, None
    if variant == "weights":
        w = 0.1 * rng.random(N)
        w[::5] = 0.0
    elif variant == "warm":
        w = 2e-2
        idx = rng.choice(N, size=24, replace=False)  # (not sorted: the ABI takes the indices in any order)
        x0 = (idx, np.where(x[idx] != 0, x[idx], 0.0) + 0.05 * rng.standard_normal(24))
    return A, b, w, x0, maxiter, alpha


@functools.lru_cache(maxsize=None)
def case_twin(case):
    A, b, w, x0, maxiter, alpha = case_args(case)
    return (fista if case[0] == "fista" else ista)(A, b, w, x0, maxiter, alpha)


def band(xt):
    """atol of the comparison with the twin result xt: entries this small on either side may differ in being zero"""
    return RTOL * float(np.max(np.abs(xt))) if len(xt) else 0.0


def compare(x, xt):
    """the parity rule: every coordinate within RTOL · max|x_twin|; the same support outside the band |x_j| ≤ atol on either side; at
    most N/100 coordinates in the band.  Prints the figures, then asserts."""
    atol = band(xt)
    err = float(np.max(np.abs(x - xt))) if len(xt) else 0.0
    inband = ((np.abs(x) <= atol) & (x != 0)) | ((np.abs(xt) <= atol) & (xt != 0))
    flips = ((x != 0) != (xt != 0)) & ~inband
    print(f"max|x - twin| = {err:.3e}  atol = {atol:.3e}  nnz = {np.count_nonzero(x)} / twin {np.count_nonzero(xt)}  "
          f"in band = {int(inband.sum())}  flips = {int(flips.sum())}")
    assert err <= atol, (err, atol)
    assert not flips.any(), np.flatnonzero(flips)[:10]
    assert inband.sum() <= len(xt) / 100, int(inband.sum())
