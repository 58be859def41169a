"""numpy Float64 restatement of csmp_bp_joint, straight from the recurrences of include/csmp.h, and the seeded cases the CPU and the GPU
tests share.  A plain helper module: the parity yardstick of tests/test_bp_joint_static.py and tests/test_gpu_bp_joint.py.

    problem     min Σ_j w_j ‖X[j, :]‖₂  subject to  A X = B:  ONE row support for all columns of B
    iteration   bp_twin's with matrices in place of vectors.  Z, U are N × nsig;  P = A Z, Q = A U, E, Y are M × nsig;  t_j = w_j / ρ
                    E = P − Q − B;   Y = G⁻¹ E  (V = R⁻ᵀE, Y = R⁻¹V);   C = Aᵀ Y;   T = Z − C
                    Z⁺ = row_shrinkage(T, t)  (ista_joint_twin's: n_j in column order, 0 exactly where !(n_j > t_j));   U⁺ = T − Z⁺
                    R = B − A Z⁺;   P⁺ = B − R;   Q⁺ = P − G Y − P⁺
                every check_every iterations: stop when ‖U⁺ − U‖_F < tol and ρ‖Z⁺ − Z‖_F < tol -- ONE rule for all columns.
The result is Z; the dictionary's values are promoted to Float64 exactly, as the library does."""
import functools
from collections import namedtuple

import numpy as np

import bp_twin
from ista_joint_twin import band, compare, row_shrinkage, rows_in_band  # noqa: F401  (the parity rule is ista_joint_twin's)

TWIN_TOL = bp_twin.TWIN_TOL
NSIG_MAX = 17


def bp_joint(A, B, w=None, rho=1.0, maxiter=16384, tol=1e-8, check_every=32, At=None, state=None):
    """(Z, info).  At: a function Y -> AᵀY in place of the matrix product (the static test reverses its summation order).
    state: a dict that receives the final U (the scaled dual: the optimality test derives Λ from it)"""
    A, G, L = bp_twin.factor(A)
    B = np.asarray(B, dtype=np.float64)
    M, N = A.shape
    nsig = B.shape[1]
    w = np.ones(N) if w is None else np.broadcast_to(np.asarray(w, dtype=np.float64), (N,))
    t = w / rho
    Li = np.linalg.solve(L, np.eye(M))  # R⁻ᵀ (lower): the device keeps the two inverse triangles and multiplies
    At = At or (lambda Y: A.T @ Y)
    Z, U, P, Q = np.zeros((N, nsig)), np.zeros((N, nsig)), np.zeros((M, nsig)), np.zeros((M, nsig))
    it, ok = 0, False
    for it in range(1, maxiter + 1):
        E = P - Q - B
        Y = Li.T @ (Li @ E)
        T = Z - At(Y)
        Zn = row_shrinkage(T, t)
        Un = T - Zn
        R = B - A @ Zn
        Pn = B - R
        Qn = P - G @ Y - Pn
        prim, dual = np.linalg.norm(Un - U), rho * np.linalg.norm(Zn - Z)
        Z, U, P, Q = Zn, Un, Pn, Qn
        if it % check_every == 0 and prim < tol and dual < tol:
            ok = True
            break
    if state is not None:
        state["U"] = U
    Z = Z + 0.0  # (−0.0 → 0.0: an exact zero is a structural zero)
    return Z, {"iterations": it, "converged": ok, "rows": int(np.any(Z != 0, axis=1).sum()),
               "resnorm": np.linalg.norm(B - A @ Z, axis=0)}


def data(M, N, k, seed, dtype=np.float64, nsig=NSIG_MAX):
    """bp_twin.data's generator for nsig columns: the same dictionary and the same k planted atoms (the same draws, in the same order),
    then amplitudes ±(0.5 … 1.5) per entry of the k planted ROWS; B = A X in Float64"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N))
    A -= 1e-6 * A.mean(axis=0, keepdims=True)
    A /= np.sqrt((A * A).sum(axis=0, keepdims=True))
    A = np.asfortranarray(A.astype(dtype))
    ind = np.sort(rng.choice(N, size=k, replace=False))
    X = np.zeros((N, nsig))
    X[ind] = rng.choice(np.array([-1.0, 1.0]), size=(k, nsig)) * (0.5 + rng.random((k, nsig)))
    return A, X, np.asfortranarray(A.astype(np.float64) @ X)


# shape cases: name -> (M, N, k, seed, dtype, weighted, maxiter)
#   twin iterations at tol = 1e-9, check_every = 32, for 1 / 2 / 3 / 5 / 8 / 9 / 17 columns (tests/test_bp_joint_static.py prints them)
SHAPES = {
    "32x48_f64": (32, 48, 3, 0, np.float64, False, 16384),
    "vertex_32x64_f64": (32, 64, 12, 4, np.float64, False, 16384),   # one column ends in a dense vertex; two or more recover the rows
    "weighted_100x257_f32": (100, 257, 10, 1, np.float32, True, 16384),
    "wide_130x1000_f32": (130, 1000, 12, 2, np.float32, False, 16384),
    "short_256x3000_f32": (256, 3000, 16, 4, np.float32, False, 16384),     # columns of two chunks: k_sweep_short
    "ragged_1000x3000_f64": (1000, 3000, 40, 5, np.float64, False, 64),     # clamped loads, the Float64 pass in chunks of four; capped
}

Case = namedtuple("Case", "shape nsig")


def parity_cases():
    """every case the GPU parity tests run.  nsig: 2 the smallest joint call, 3 a remainder chunk, 5 crosses the Float64 pass's chunk of
    4, 8 a full chunk, 9 and 17 one and two columns past it"""
    c = [Case("32x48_f64", n) for n in (2, 3, 5, 8, 9, 17)]
    c += [Case("wide_130x1000_f32", n) for n in (2, 3, 5, 8, 9, 17)]
    c += [Case("vertex_32x64_f64", 8), Case("vertex_32x64_f64", 17), Case("weighted_100x257_f32", 9), Case("short_256x3000_f32", 17),
          Case("ragged_1000x3000_f64", 9)]
    return c


def case_id(c):
    return f"{c.shape}-n{c.nsig}"


@functools.lru_cache(maxsize=None)
def shape_data(shape):
    """(A, X planted, B with NSIG_MAX columns, w or None, maxiter): a case takes the first nsig columns"""
    M, N, k, seed, dtype, weighted, maxiter = SHAPES[shape]
    A, X, B = data(M, N, k, seed, dtype)
    w = np.random.default_rng(1000 + seed).uniform(0.5, 2.0, N) if weighted else None
    return A, X, B, w, maxiter


def case_args(c):
    """(A, B, w, maxiter) of a parity case"""
    A, _, Ball, w, maxiter = shape_data(c.shape)
    return A, np.asfortranarray(Ball[:, :c.nsig]), w, maxiter


@functools.lru_cache(maxsize=None)
def case_twin(c):
    A, B, w, maxiter = case_args(c)
    return bp_joint(A, B, w, maxiter=maxiter, tol=TWIN_TOL)
