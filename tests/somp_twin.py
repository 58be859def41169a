"""A numpy Float64 statement of simultaneous OMP (S-OMP: Tropp, Gilbert and Strauss 2006) as csmp_somp runs it -- omp's driver
(src/matchingpursuit.jl:62-82 of the reference) with the residual matrix R in place of r and ONE CGS2 factorisation -- and the inputs
of the somp tests, built from seeds: unit-norm Gaussian dictionaries, six planted rows shared by all columns, 5 % noise.

    somp(A, B, eps, k, p)   -> Twin(order, support, X, hist, margins, resnorm)
    cases()                 -> every (name, A, B, k, p) the GPU tests solve; tests/test_somp_static.py checks that no pick of any of
                               them is a near-tie in the twin, so a pick the device makes differently is a defect and not a tie
"""
import collections
import functools

import numpy as np

Twin = collections.namedtuple("Twin", "order support X hist margins resnorm")
Case = collections.namedtuple("Case", "name A B k p")


def somp(A, B, eps, k, p=1):
    """order: the atoms as they were picked; support: ascending; X: len(support) x nsig, row i the coefficients of support[i];
    hist[t]: ||R||_F after update t + 1; margins[t]: (s_best - s_second) / s_best of pick t; resnorm: ||r_l|| at the end."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    M, N = A.shape
    nsig = B.shape[1]
    R = B.copy()
    Q = np.zeros((M, k))
    Rf = np.zeros((k, k))
    Z = np.zeros((k, nsig))
    order, hist, margins = [], [], []
    for t in range(k):
        if t > 0:
            f2 = 0.0
            for l in range(nsig):               # ||R||_F^2 in column order
                f2 += float(R[:, l] @ R[:, l])
            if not np.sqrt(f2) >= eps:          # norm(residual) >= eps || break
                break
        C = A.T @ R
        s = np.zeros(N)
        for l in range(nsig):                   # the scores in column order
            s += np.abs(C[:, l]) if p == 1 else C[:, l] ** 2
        i = int(np.argmax(s))                   # the lowest index among equals
        j = len(order)
        if j >= M or j >= k or i in order:      # omp's guards; a pick inside the support ends the solve
            break
        second = np.partition(s, -2)[-2] if N > 1 else 0.0
        margins.append(float((s[i] - second) / s[i]) if s[i] > 0 else 0.0)
        a = A[:, i]
        w1 = Q[:, :j].T @ a                     # CGS2
        v = a - Q[:, :j] @ w1
        w2 = Q[:, :j].T @ v
        v = v - Q[:, :j] @ w2
        rho = float(np.linalg.norm(v))
        q = v / rho
        Q[:, j] = q
        Rf[:j, j] = w1 + w2
        Rf[j, j] = rho
        z = q @ R
        Z[j] = z
        R -= np.outer(q, z)
        order.append(i)
        hist.append(float(np.linalg.norm(R)))
    n = len(order)
    X = np.linalg.solve(Rf[:n, :n], Z[:n]) if n else np.zeros((0, nsig))
    perm = np.argsort(order, kind="stable")
    return Twin(np.asarray(order, np.int64), np.asarray(order, np.int64)[perm], X[perm], np.asarray(hist), np.asarray(margins),
                np.linalg.norm(R, axis=0))


# ---- the inputs
ROWS, NOISE, K = 6, 0.05, 12
NSIGS = (1, 2, 4, 5, 8, 9, 17)
PS = (1, 2)
SHAPES = {"f32": (1024, 3000, np.float32, 101), "f32_ragged": (1001, 2999, np.float32, 102), "f64": (512, 1500, np.float64, 103)}
LONG = ("f64", 3, 260)                        # (shape, nsig, k): the finish beyond 256 columns
PHASED = (32768, 520, np.float32, 104, 3, 4)  # (M, N, dtype, seed, nsig, k): no shared pass
ALLOC = (256, 1024, np.float32, 105, 9, 6)    # the failed allocations
EPS_CASE = ("f32", 5, 1)                      # (shape, nsig, p): the eps stop


@functools.lru_cache(maxsize=None)
def planted(M, N, dtype, seed, nsig):
    """(A, B): A unit-norm Gaussian columns in `dtype`, column-major; B = A[:, S] X + 5 % noise per column, Float64, six rows S shared"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    A = np.asfortranarray(A.astype(dtype))
    S = np.sort(rng.choice(N, ROWS, replace=False))
    X = rng.standard_normal((ROWS, nsig))
    X += np.sign(X)                              # every planted coefficient at least 1 in magnitude
    B = A[:, S].astype(np.float64) @ X
    E = rng.standard_normal((M, nsig))
    B += NOISE * E * (np.linalg.norm(B, axis=0) / np.linalg.norm(E, axis=0))
    A.setflags(write=False)
    B = np.asfortranarray(B)
    B.setflags(write=False)
    return A, B


def shape_data(name):
    M, N, dtype, seed = SHAPES[name]
    return planted(M, N, dtype, seed, max(NSIGS))


def columns(B, nsig):
    return np.asfortranarray(B[:, :nsig])


def copies():
    A, B = shape_data("f32")
    return A, np.asfortranarray(np.stack([B[:, 0]] * 3, axis=1))


def cases():
    out = []
    for name in SHAPES:
        A, B = shape_data(name)
        for nsig in NSIGS:
            for p in PS:
                out.append(Case(f"{name}-{nsig}-p{p}", A, columns(B, nsig), K, p))
    A, B = shape_data(LONG[0])
    out.append(Case("long", A, columns(B, LONG[1]), LONG[2], 1))
    M, N, dtype, seed, nsig, k = PHASED
    out.append(Case("phased", *planted(M, N, dtype, seed, nsig), k, 1))
    M, N, dtype, seed, nsig, k = ALLOC
    out.append(Case("alloc", *planted(M, N, dtype, seed, nsig), k, 1))
    out.append(Case("copies", *copies(), K, 1))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, eps=0.0):
    """the twin's solve of case `name`, computed once"""
    c = {c.name: c for c in cases()}[name]
    return somp(c.A, c.B, eps, c.k, c.p)
