"""numpy Float64 twin of the dictionary analysis (csmp_colnorms, csmp_cumbabel), written from the formulas of include/csmp.h:

    g_i = |Aᵀ a_i| with g_i[i] = 0;  s_i(m) = the sum of the m largest entries of g_i;  μ₁(m) = max_i s_i(m),  m = 1..k
    normalize: every entry is |⟨a_i, a_j⟩| / (‖a_i‖ ‖a_j‖), 0 where a column is zero
    pair: the columns (i, j), i < j, that attain μ₁(1) -- the lowest i, then the lowest j among equals; (-1, -1) when N = 1

by the full N x N Gram matrix (which the library never forms), and the bound the GPU tests hold the library to."""
import functools

import numpy as np

U = 2.0 ** -53


def gamma(n):
    """γ(n) = n u / (1 - n u), u = 2⁻⁵³: the relative error bound of n Float64 roundings in a row"""
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def gram_abs(A, normalize=False):
    """|AᵀA| in Float64 on the exactly promoted values, the diagonal set to zero; under normalize divided by ‖a_i‖ ‖a_j‖"""
    A = np.asarray(A, dtype=np.float64)
    G = np.abs(A.T @ A)
    if normalize:
        n = np.linalg.norm(A, axis=0)
        s = np.divide(1.0, n, out=np.zeros_like(n), where=n > 0)
        G = G * np.outer(s, s)
    np.fill_diagonal(G, 0.0)
    return G


def cumbabel(A, k, normalize=False):
    G = gram_abs(A, normalize)
    top = -np.sort(-G, axis=1)[:, :k]  # the k largest of every row, descending (the self entry is one of the zeros)
    return np.cumsum(top, axis=1).max(axis=0)


def babel(A, k, normalize=False):
    return cumbabel(A, k, normalize)[k - 1]


def coherence(A, normalize=False):
    return babel(A, 1, normalize)


def pair(A, normalize=False):
    G = gram_abs(A, normalize)
    N = G.shape[0]
    if N == 1:
        return (-1, -1)
    iu = np.triu_indices(N, 1)  # row-major: ascending i, then ascending j
    v = G[iu]
    t = int(np.argmax(v))  # the FIRST maximum
    return (int(iu[0][t]), int(iu[1][t]))


def top1_gap(A, normalize=False):
    """the largest entry above the diagonal minus the second largest"""
    G = gram_abs(A, normalize)
    v = np.sort(G[np.triu_indices(G.shape[0], 1)])
    return float(v[-1] - v[-2])


def cumbabel_by_columns(A, k):
    """the loop of src/util.jl:106-113, one column at a time"""
    A = np.asarray(A, dtype=np.float64)
    mu = np.zeros(k)
    for i in range(A.shape[1]):
        inner = np.abs(A.T @ A[:, i])
        inner[i] = 0.0
        inner = np.sort(inner)[::-1][:k]
        mu = np.maximum(mu, np.cumsum(inner))
    return mu


def tolerance(A, mu, normalize=False):
    """|Δμ₁(m)| ≤ 2 m γ(M + 8) S + 2 γ(m) μ₁(m), S = max_j ‖a_j‖² (1 under normalize): any order of fused or unfused Float64
    accumulation of an inner product errs by at most γ(M) ‖a_i‖ ‖a_j‖, a top-m sum is m-Lipschitz in the sup norm, the running sum
    adds γ(m) of itself, and there are two sides (the library and this twin)."""
    A = np.asarray(A, dtype=np.float64)
    M = A.shape[0]
    S = 1.0 if normalize else float((A * A).sum(axis=0).max())
    m = np.arange(1, len(mu) + 1, dtype=np.float64)
    return 2.0 * m * gamma(M + 8) * S + 2.0 * gamma(m) * np.asarray(mu)


# ------------------------------------------------------------------------------------------ the GPU parity cases
# (M, N, dtype, ks): one partial strip with k = N-1 and k = N; ragged rows and three strips, the last with ONE query; the cap;
# 64 row blocks; a ragged last row block over two strips; long columns
PARITY_CASES = [
    (32, 48, "f64", (47, 48)),
    (100, 257, "f32", (7,)),
    (256, 1000, "f32", (64,)),
    (64, 1500, "f64", (1024,)),
    (4096, 300, "f32", (299,)),
    (8200, 130, "f32", (5,)),
    (20000, 200, "f64", (1,)),
]


def case_id(c):
    return f"{c[0]}x{c[1]}_{c[2]}"


@functools.lru_cache(maxsize=None)
def random_dictionary(M, N, dtype, seed=0):
    """Gaussian columns of norm about 1 (not exactly: normalize has something to do); read-only"""
    rng = np.random.default_rng(1000 * seed + M + N)
    A = rng.standard_normal((M, N)) / np.sqrt(M)
    A = np.asfortranarray(A.astype(np.float32 if dtype == "f32" else np.float64))
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def case_twin(M, N, dtype, k, normalize):
    mu = cumbabel(random_dictionary(M, N, dtype), k, normalize)
    mu.setflags(write=False)
    return mu


def integer_dictionary(M, N, dtype, seed, planted):
    """entries in {-2..2}: every product and every sum is exact in Float64.  planted: columns duplicated and negated so that several
    pairs tie for the largest inner product"""
    rng = np.random.default_rng(seed)
    A = rng.integers(-2, 3, size=(M, N)).astype(np.float32 if dtype == "f32" else np.float64)
    if planted:
        heavy = np.full(M, 2.0)
        heavy[::2] = -2.0  # ‖heavy‖² = 4 M: no random pair reaches it
        for i, j, sign in ((5, 77, 1.0), (3, 129 if N > 129 else N - 1, -1.0), (40, 41, 1.0), (3, 60, 1.0)):
            A[:, i] = heavy
            A[:, j] = sign * heavy
    return np.asfortranarray(A)
