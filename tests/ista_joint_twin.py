"""numpy Float64 restatement of ista_joint / fista_joint, straight from the formulas of include/csmp.h (csmp_ista_joint), and the seeded
parity cases the CPU and the GPU tests share.  A plain helper module: the parity yardstick of tests/test_ista_joint_static.py and
tests/test_gpu_ista_joint.py.

    objective   ‖B − A X‖_F² + Σ_j w_j ‖X[j, :]‖₂
    step        R = B − A Y,  C = Aᵀ R,  U = Y + 2α C,  n_j = √(Σ_l U[j,l]²) added in column order,  t_j = w_j α,  α = stepsize
    X⁺[j, :]    0 where !(n_j > t_j), else (1 − t_j / n_j) U[j, :]
    ISTA        Y = X
    FISTA       t₁ = 1,  t⁺ = (1 + √(1 + 4t²))/2,  Y⁺ = X⁺ + ((t − 1)/t⁺)(X⁺ − X),  Y₁ = X₀
Exactly maxiter iterations; the dictionary's values are promoted to Float64 exactly, as the library does."""
import functools
from collections import namedtuple

import numpy as np

import ista_twin

RTOL = ista_twin.RTOL  # the suite's tolerance: |X − X_twin| ≤ RTOL · max|X_twin| for every entry


def row_shrinkage(U, t):
    n2 = np.zeros(U.shape[0])
    for l in range(U.shape[1]):  # column order
        n2 = n2 + U[:, l] * U[:, l]
    n = np.sqrt(n2)
    live = n > t
    scale = np.zeros_like(n)
    scale[live] = 1.0 - t[live] / n[live]
    X = scale[:, None] * U
    X[~live] = 0.0
    return X


def _start(A, B, lam_or_w, X0):
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    w = ista_twin.weights(lam_or_w, A.shape[1])
    X = np.zeros((A.shape[1], B.shape[1])) if X0 is None else np.array(X0, dtype=np.float64)
    return A, B, w, X


def ista_joint(A, B, lam_or_w, X0=None, maxiter=1024, stepsize=1e-2, At=None):
    """At: a function R -> AᵀR in place of the matrix product (the static test reverses its summation order)"""
    A, B, w, X = _start(A, B, lam_or_w, X0)
    At = At or (lambda R: A.T @ R)
    for _ in range(maxiter):
        X = row_shrinkage(X + 2 * stepsize * At(B - A @ X), w * stepsize)
    return X + 0.0  # (−0.0 → 0.0: an exact zero is a structural zero)


def fista_joint(A, B, lam_or_w, X0=None, maxiter=1024, stepsize=1e-2, At=None):
    A, B, w, X = _start(A, B, lam_or_w, X0)
    At = At or (lambda R: A.T @ R)
    Y, t = X.copy(), 1.0
    for _ in range(maxiter):
        Xn = row_shrinkage(Y + 2 * stepsize * At(B - A @ Y), w * stepsize)
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        Y = Xn + ((t - 1.0) / tn) * (Xn - X)
        X, t = Xn, tn
    return X + 0.0


def objective(A, B, lam_or_w, X):
    A = np.asarray(A, dtype=np.float64)
    R = np.asarray(B, dtype=np.float64) - A @ X
    return float(np.sum(R * R) + ista_twin.weights(lam_or_w, A.shape[1]) @ np.linalg.norm(X, axis=1))


def planted(M, N, k, dtype, seed, nsig, noise=5e-3):
    """unit-norm Gaussian columns (normalised in Float64, then rounded to dtype), k planted rows shared by all nsig columns with
    amplitudes ±(0.5 … 1.5), B = A X + noise"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0)
    A = np.asfortranarray(A.astype(dtype))
    X = np.zeros((N, nsig))
    S = rng.choice(N, size=k, replace=False)
    X[S] = rng.choice([-1.0, 1.0], size=(k, nsig)) * (0.5 + rng.random((k, nsig)))
    B = A.astype(np.float64) @ X + noise * rng.standard_normal((M, nsig))
    return A, X, np.asfortranarray(B.astype(dtype))


NSIG_MAX = 17
# shape cases: name -> (M, N, k, dtype, seed, maxiter)
SHAPES = {
    "32x48_f64": (32, 48, 3, np.float64, 1, 512),
    "256x1024_f32": (256, 1024, 16, np.float32, 2, 512),
    "short_256x3000_f32": (256, 3000, 16, np.float32, 4, 256),     # columns of two chunks: k_sweep_short
    "ragged_1000x3000_f64": (1000, 3000, 40, np.float64, 5, 256),
    "long_32768x96_f32": (32768, 96, 8, np.float32, 6, 32),         # a residual longer than the LDS: no shared pass, one sweep per column
}

Case = namedtuple("Case", "method shape nsig variant maxiter")  # variant: a λ, "weights" or "warm"; maxiter None: the shape's


def parity_cases():
    """every case the GPU parity tests run.  nsig: 2 the smallest group, 3 a remainder chunk, 8 a full chunk, 9 and 17 one and two
    columns past it; 5 crosses the Float64 pass's chunk of 4.  FISTA at λ ≥ 2e-2 only, as ista_twin restricts it."""
    c = [Case("ista", "32x48_f64", n, 2e-2, None) for n in (2, 3, 5, 8, 9, 17)]
    c += [Case("ista", "32x48_f64", 9, 1e-3, None), Case("fista", "32x48_f64", 5, 0.2, None), Case("fista", "32x48_f64", 9, 2e-2, None)]
    c += [Case("ista", "256x1024_f32", n, 2e-2, None) for n in (2, 3, 8, 9, 17)]
    c += [Case("ista", "256x1024_f32", 9, 1e-3, None), Case("ista", "256x1024_f32", 9, 0.2, None), Case("fista", "256x1024_f32", 9, 2e-2, None),
          Case("fista", "256x1024_f32", 17, 0.2, None), Case("ista", "256x1024_f32", 9, "weights", None),
          Case("fista", "256x1024_f32", 9, "weights", None), Case("fista", "256x1024_f32", 9, "warm", None)]
    c += [Case("ista", "short_256x3000_f32", 17, 2e-2, None), Case("ista", "short_256x3000_f32", 8, 1e-3, None),
          Case("fista", "short_256x3000_f32", 3, 0.2, None)]
    c += [Case("ista", "ragged_1000x3000_f64", 3, 2e-2, None), Case("fista", "ragged_1000x3000_f64", 2, 2e-2, None),
          Case("ista", "ragged_1000x3000_f64", 9, 0.2, 64), Case("ista", "ragged_1000x3000_f64", 5, "warm", 64)]
    c += [Case("ista", "long_32768x96_f32", 3, 2e-2, None), Case("fista", "long_32768x96_f32", 3, 0.2, None)]
    return c


def case_id(c):
    return f"{c.method}-{c.shape}-n{c.nsig}-{c.variant}" + (f"-it{c.maxiter}" if c.maxiter else "")


@functools.lru_cache(maxsize=None)
def shape_data(shape):
    """(A, X planted, B with NSIG_MAX columns, stepsize, maxiter): a case takes the first nsig columns"""
    M, N, k, dtype, seed, maxiter = SHAPES[shape]
    A, X, B = planted(M, N, k, dtype, seed, NSIG_MAX)
    return A, X, B, ista_twin.stepsize(A), maxiter


def case_args(c):
    """(A, B, w, X0, maxiter, stepsize) of a parity case.  "weights": a weight vector between 0 and 0.1 with every fifth weight exactly
    zero; "warm": λ = 2e-2 from a dense warm start with 24 non-zero rows (some planted, some not)."""
    A, X, Ball, alpha, maxiter = shape_data(c.shape)
    N = A.shape[1]
    B = np.asfortranarray(Ball[:, :c.nsig])
    rng = np.random.default_rng(3000 + SHAPES[c.shape][4])
    w, X0 = c.variant, None
    if c.variant == "weights":
        w = 0.1 * rng.random(N)
        w[::5] = 0.0
    elif c.variant == "warm":
        w = 2e-2
        rows = rng.choice(N, size=24, replace=False)
        X0 = np.zeros((N, c.nsig), order="F")
        X0[rows] = X[rows, :c.nsig] + 0.05 * rng.standard_normal((24, c.nsig))
    return A, B, w, X0, c.maxiter or maxiter, alpha


@functools.lru_cache(maxsize=None)
def case_twin(c):
    A, B, w, X0, maxiter, alpha = case_args(c)
    return (fista_joint if c.method == "fista" else ista_joint)(A, B, w, X0, maxiter, alpha)


def band(Xt):
    """atol of the comparison with the twin result Xt: rows this small on either side may differ in being zero"""
    return RTOL * float(np.max(np.abs(Xt))) if Xt.size else 0.0


def rows_in_band(X, atol):
    n = np.linalg.norm(X, axis=1)
    return (n <= atol) & (n != 0)


def compare(X, Xt):
    """the parity rule, ista_twin.compare's per row: every entry within RTOL · max|X_twin|; the same row support outside the band
    ‖row‖ ≤ atol on either side; at most N/100 rows in the band.  Prints the figures, then asserts."""
    assert X.shape == Xt.shape
    atol = band(Xt)
    err = float(np.max(np.abs(X - Xt))) if Xt.size else 0.0
    inband = rows_in_band(X, atol) | rows_in_band(Xt, atol)
    nz, nzt = np.any(X != 0, axis=1), np.any(Xt != 0, axis=1)
    flips = (nz != nzt) & ~inband
    print(f"max|X - twin| = {err:.3e}  atol = {atol:.3e}  rows = {int(nz.sum())} / twin {int(nzt.sum())}  "
          f"in band = {int(inband.sum())}  flips = {int(flips.sum())}")
    assert err <= atol, (err, atol)
    assert not flips.any(), np.flatnonzero(flips)[:10]
    assert inband.sum() <= X.shape[0] / 100, int(inband.sum())
