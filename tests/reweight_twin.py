"""numpy Float64 restatement of the reweighted l1 path, straight from the formulas of include/csmp.h (csmp_ard_weights,
csmp_ista_reweighted), and the seeded cases the CPU and the GPU tests share.  A plain helper module: the parity yardstick of
tests/test_reweight_static.py and tests/test_gpu_reweight.py.  Nothing here reads the reference.

    Candès      w_j = 1 / (|x_j| + ε)
    ARD         iter times:  d = |x| ./ w;  K = εI + A diag(d) Aᵀ;  w_j = √max(a_jᵀ K⁻¹ a_j, 0)
                restated twice -- ard_direct solves with the M × M K itself, ard_support with the k × k matrix of the support:
                L Lᵀ = ε diag(w_S ./ |x_S|) + A_SᵀA_S,  a_jᵀ K⁻¹ a_j = (‖a_j‖² − ‖L⁻¹A_Sᵀa_j‖²) / ε
    outer loop  x = solve(1);  for i = 2 … maxiter:  w from x;  xs = solve(w), warm-started from x;  ‖xs − x‖ < min_decrease: return xs;
                x = xs        (solve(w) = ista / fista on ‖b − A x‖² + λ Σ w_j |x_j|)
"""
import functools

import numpy as np

import ista_twin as tw
from analysis_twin import gamma

CANDES, ARD = 0, 1
SCHEMES = {"candes": CANDES, "ard": ARD}
ARD_KMAX = 1024  # CSMP_ARD_KMAX


def candes_weights(x, eps):
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"eps = {eps} has to be positive and finite")
    w = 1.0 / (np.abs(np.asarray(x, dtype=np.float64)) + eps)
    if not np.all(np.isfinite(w)):
        raise ValueError("weights contain NaN or Inf")
    return w


def _ard_args(A, x, w, eps, iter, kmax=None):
    A = np.asarray(A, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(A.shape[1]) if w is None else np.array(w, dtype=np.float64)
    if x.shape != (A.shape[1],) or w.shape != x.shape:
        raise ValueError("length(x) and length(w) have to be size(A, 2)")
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"eps = {eps} has to be positive and finite")
    if iter < 1:
        raise ValueError(f"iter = {iter} has to be at least 1")
    if not np.all((w > 0) & np.isfinite(w)):
        raise ValueError("weights cannot be zero (every weight has to be positive and finite)")
    if not np.all(np.isfinite(x)):
        raise ValueError("x has to be finite")
    kmax = min(A.shape[0], ARD_KMAX) if kmax is None else kmax
    if np.count_nonzero(x) > kmax:
        raise IndexError(f"nnz(x) = {np.count_nonzero(x)} but at most {kmax} are taken")
    return A, x, w


def ard_direct(A, x, w=None, eps=1e-2, iter=8, return_K=False):
    """the reference's formulation: the M × M matrix K, a solve per atom"""
    A, x, w = _ard_args(A, x, w, eps, iter)
    K = None
    for _ in range(iter):
        d = np.abs(x) / w
        K = eps * np.eye(A.shape[0]) + (A * d) @ A.T
        q = np.einsum("ij,ij->j", A, np.linalg.solve(K, A))
        w = np.sqrt(np.maximum(q, 0.0))
    return (w, K) if return_K else w


def ard_support(A, x, w=None, eps=1e-2, iter=8, kmax=None):
    """the library's formulation: the k × k matrix of the support; iterations 1 … iter−1 update w_S only.  kmax: the largest support
    taken, min(M, ARD_KMAX) as csmp_ard_weights; the outer loop passes ARD_KMAX (an iterate of ista may have more than M non-zeros)."""
    A, x, w = _ard_args(A, x, w, eps, iter, kmax)
    S = np.flatnonzero(x)
    n2 = np.einsum("ij,ij->j", A, A)
    if len(S) == 0:
        return np.sqrt(n2 / eps)
    AS = A[:, S]
    G = AS.T @ AS
    xS, wS = np.abs(x[S]), w[S].copy()
    for it in range(iter):
        L = np.linalg.cholesky(G + np.diag(eps * wS / xS))
        if it + 1 < iter:
            Y = np.linalg.solve(L, G)
            wS = np.sqrt(np.maximum((np.diag(G) - np.einsum("ij,ij->j", Y, Y)) / eps, 0.0))
    Y = np.linalg.solve(L, AS.T @ A)
    return np.sqrt(np.maximum((n2 - np.einsum("ij,ij->j", Y, Y)) / eps, 0.0))


def ard_tolerance(A, x, w=None, eps=1e-2, iter=8):
    """the bound on |Δ w_j²|, per atom: B_j = γ(8(M + k)) · κ₂(K) · ‖a_j‖² / ε for iter = 1 -- a Cholesky solve plus the subtraction of
    two O(‖a_j‖²) terms, divided by ε --, (1 + κ) · B_j for iter > 1 (the earlier iterations' relative errors in d enter the last K).
    κ is that of the LAST K, taken from the direct restatement by eigvalsh.  Returns (bound, κ)."""
    A64 = np.asarray(A, dtype=np.float64)
    _, K = ard_direct(A, x, w, eps, iter, return_K=True)
    ev = np.linalg.eigvalsh(K)
    kappa = float(ev[-1] / ev[0])
    M, k = A64.shape[0], np.count_nonzero(x)
    B = gamma(8 * (M + k)) * kappa * np.einsum("ij,ij->j", A64, A64) / eps
    return (B if iter == 1 else (1.0 + kappa) * B), kappa


def compare_weights(w, wt, bound, what=""):
    """|w² − w_twin²| ≤ bound for every atom; prints the largest error beside its bound, then asserts"""
    err = np.abs(np.asarray(w) ** 2 - wt ** 2)
    j = int(np.argmax(err / bound))
    print(f"{what}: max |Δw²| / bound = {err[j] / bound[j]:.3e}  (|Δw²| = {err[j]:.3e}, bound = {bound[j]:.3e}, atom {j})")
    assert np.all(np.isfinite(w)) and np.all(err <= bound), (j, err[j], bound[j])


def reweighted(A, b, lam, scheme, eps=1e-2, ard_iter=8, maxiter=8, min_decrease=1e-8, inner_maxiter=1024, stepsize=1e-2, accel=False):
    """(x, w, solves done, [‖xs − x‖ of every re-solve], (x, w) the last reweighting started from)"""
    if scheme not in (CANDES, ARD):
        raise ValueError("scheme")
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"eps = {eps} has to be positive and finite")
    if ard_iter < 1 or maxiter < 1:
        raise ValueError("ard_iter and maxiter have to be at least 1")
    if not min_decrease >= 0:
        raise ValueError("min_decrease has to be non-negative")
    A64 = np.asarray(A, dtype=np.float64)
    N = A64.shape[1]
    solve = tw.fista if accel else tw.ista
    x = solve(A64, b, lam, None, inner_maxiter, stepsize)
    w = np.ones(N)
    done, hist, last = 1, [], None
    for _ in range(2, maxiter + 1):
        last = (x, w)
        w = candes_weights(x, eps) if scheme == CANDES else ard_support(A64, x, w, eps, ard_iter, kmax=ARD_KMAX)
        nz = np.flatnonzero(x)
        xs = solve(A64, b, lam * w, (nz, x[nz]), inner_maxiter, stepsize)
        done += 1
        hist.append(float(np.linalg.norm(xs - x)))
        x = xs
        if hist[-1] < min_decrease:
            break
    return x, w, done, hist, last


# ---------------------------------------------------------------------------------------------- shared cases
LAMBDA, EPS, OUTER = 2e-2, 1e-2, 8
SOLVE_SHAPES = ("32x48_f64", "256x1024_f32", "short_256x3000_f64")  # of ista_twin.SHAPES


@functools.lru_cache(maxsize=None)
def solve_twin(shape, scheme, accel, min_decrease=0.0):
    A, _, b, alpha, inner = tw.case_data(shape)
    return reweighted(A, b, LAMBDA, SCHEMES[scheme], EPS, 8, OUTER, min_decrease, inner, alpha, accel)


def _planted_x(N, S, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros(N)
    x[S] = rng.choice([-1.0, 1.0], size=len(S)) * (0.5 + rng.random(len(S)))
    return x


# weight cases: name -> (M, N, dtype, seed, support); the support "planted" is that of ista_twin.planted's signal (k atoms)
WEIGHT_CASES = {
    "32x48_f64_k3": (32, 48, np.float64, 1, 3),            # M below one 64-row block
    "256x1024_f32_k16": (256, 1024, np.float32, 2, 16),
    "261x1000_f32_k150": (261, 1000, np.float32, 7, 150),  # two direction blocks (128 | 22), a ragged last row block (5 rows), N % 128 != 0
    "261x1000_f64_k150": (261, 1000, np.float64, 7, 150),
    "1000x300_f64_k130": (1000, 300, np.float64, 8, 130),  # 128 | 2
    "64x256_f64_k0": (64, 256, np.float64, 9, 0),
    "64x256_f64_k1": (64, 256, np.float64, 9, 1),
    "64x256_f32_ends": (64, 256, np.float32, 10, "ends"),  # a support containing atoms 0 and N - 1
}


@functools.lru_cache(maxsize=None)
def weight_case(name):
    """(A, x, w_in random in [0.5, 2])"""
    M, N, dtype, seed, k = WEIGHT_CASES[name]
    A, _, _ = tw.planted(M, N, 1, dtype, seed)
    rng = np.random.default_rng(500 + seed)
    if k == "ends":
        S = np.array([0, 17, 100, N - 1])
    else:
        S = np.sort(rng.choice(N, size=k, replace=False))
    x = _planted_x(N, S, 900 + seed)
    return A, x, 0.5 + 1.5 * rng.random(N)


@functools.lru_cache(maxsize=None)
def weight_twin(name, iter, ones):
    """(w of ard_support, bound on |Δw²|, κ)"""
    A, x, w_in = weight_case(name)
    w0 = None if ones else w_in
    bound, kappa = ard_tolerance(A, x, w0, EPS, iter)
    return ard_support(A, x, w0, EPS, iter), bound, kappa
