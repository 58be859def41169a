"""Host-side mirror of the reference's matching-pursuit interface, over libcsmp.so.

Same names, argument meaning and error behaviour as the reference (paths relative to it):

    mp(A, b, k[, x])                         src/matchingpursuit.jl:34-40
    omp(A, b, k) / omp(A, b, eps, k) / omp(A, b; max_residual, sparsity)   :73-91
    gomp(A, b, l, k) / gomp(A, b, l, eps, k) / gomp(A, b, l; ...)          :126-148
    sp(A, b, k, delta=1e-12; maxiter=16k)    src/twostage.jl:87-101
    fr(A, b, max_eps, min_delta, k) / fr(A, b; max_residual, min_decrease, sparsity) = ols = oomp = ormp
                                             src/forward.jl:34-54
    FR functor with update!                  src/forward.jl:88-95
    srr(A, b, k, delta=1e-12; maxiter=4k, initialization=1, l=1)          src/twostage.jl:3-33
    rmp(A, b, delta, maxiter=1) / rmp(A, b, k) / foba(A, b, delta)        src/stepwise.jl:5-56
    br / fbr / lace (A, b, max_eps, max_delta, k) and keyword forms       src/backward.jl:27-41,148-162,226-242
    ompr(A, b, k, delta; maxiter)            src/twostage.jl:184-202
    MP / OMP / GOMP functors with update!    src/matchingpursuit.jl:10-31,44-70,95-123
    argmaxinner!(P[, k])                     src/matchingpursuit.jl:181-193
    ista(A, b, λ | w[, x]; maxiter, stepsize) / fista(...) / shrinkage(x, α)   src/basispursuit.jl:144,164-204
    bp(A, b[, w]) = basispursuit / bp_candes(A, b, ε) / bp_ard(A, b, ε)         src/basispursuit.jl:1-74
    bpd(A, b, δ[, w]) = basis_pursuit_denoising / bpd_candes(A, b, δ[, ε]) / bpd_ard(A, b, δ[, ε])   src/basispursuit.jl:76-124
    sbl(A, b, σ²; maxiter, min_change) / SBL functor with update! (scalar σ²)  src/sbl.jl:1-51
    fsbl(A, b, σ²; maxiter, min_increase) / rmps(A, b, σ²; ...) / FSBL functor with update! (scalar σ²)  src/sbl.jl:57-437
    colnorms(A) / coherence(A) / babel(A, k) / cumbabel(A, k)               src/util.jl:2,96-115

`A` is either a numpy matrix (uploaded to HBM for the duration of the call) or a `Dictionary`
(uploaded once, resident -- what a caller looping over many signals wants).  Results are
`SparseVector`s with 0-based sorted `nzind`.  The reference throws bare strings
(`throw("eps = ... has to be non-negative")`); here those become ValueError with the same text.
There is no CPU path: without libcsmp.so and an MI355X every call raises `CsmpError`.
"""
import numpy as np

from . import _lib
from ._lib import CsmpError
from .sparsevec import SparseVector, spzeros


class Dictionary:
    """The measurement matrix resident in HBM (the `A` field of MP/OMP/GOMP/SP)."""

    def __init__(self, A, device=0, streamed=False):
        """A: numpy matrix / torch CUDA tensor of atoms (see Context.set_dictionary), or the path of a dictionary file.
        streamed=True: A stays in host memory and is read over the host link by every sweep -- a dictionary larger than HBM."""
        self.ctx = _lib.Context(device)
        if isinstance(A, (str, bytes)) or hasattr(A, "__fspath__"):
            self.ctx.set_dictionary_file(A, streamed=streamed)
        else:
            self.ctx.set_dictionary(A, streamed=streamed)
        self.shape = (self.ctx.M, self.ctx.N)
        self.dtype = np.dtype(self.ctx.dtype)

    @property
    def eps(self):  # eps(eltype(A)): the drivers' default tolerance (:85,89,142,146)
        return float(np.finfo(self.dtype).eps)

    def close(self):
        self.ctx.close()


def _dict(A):
    return (A, False) if isinstance(A, Dictionary) else (Dictionary(A), True)


def _meta(A):
    """(M, N, eps(eltype(A))) without touching the GPU, so argument errors surface first."""
    if isinstance(A, Dictionary):
        return A.shape[0], A.shape[1], A.eps
    A = np.asarray(A) if not hasattr(A, "dtype") else A
    if A.ndim != 2:
        raise ValueError("A must be a matrix")
    dt = np.dtype(A.dtype) if A.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    return A.shape[0], A.shape[1], float(np.finfo(dt).eps)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_eps(eps):
    if not eps >= 0:
        raise ValueError(f"ε = {eps} has to be non-negative")  # src/matchingpursuit.jl:74,127


# ------------------------------------------------------------------------------------ drivers
def omp(A, b, *args, max_residual=None, sparsity=None):
    """omp(A,b,k) | omp(A,b,eps[,k]) | omp(A,b; max_residual=eps(T), sparsity=min(size(A)...))"""
    M, N, eps0 = _meta(A)
    if len(args) == 0:  # keyword form :88-91
        eps = eps0 if max_residual is None else max_residual
        k = min(M, N) if sparsity is None else sparsity
    elif len(args) == 1 and _is_int(args[0]):  # omp(A,b,k::Int) :84-86
        eps, k = eps0, args[0]
    elif len(args) == 1:  # omp(A,b,eps) with k = size(A,1) :73
        eps, k = args[0], M
    elif len(args) == 2:
        eps, k = args
    else:
        raise TypeError("omp(A, b, [eps,] k)")
    _check_eps(eps)
    D, tmp = _dict(A)
    try:
        idx, val, _ = D.ctx.omp(b, int(k), float(eps))
        return SparseVector(N, idx, val)
    finally:
        if tmp:
            D.close()


def gomp(A, b, l, *args, max_residual=None, sparsity=None):
    """gomp(A,b,l,k) | gomp(A,b,l,eps[,k]) | gomp(A,b,l; max_residual=eps(T), sparsity=size(A,2))"""
    M, N, eps0 = _meta(A)
    if len(args) == 0:  # :145-148
        eps = eps0 if max_residual is None else max_residual
        k = N if sparsity is None else sparsity
    elif len(args) == 1 and _is_int(args[0]):  # :141-143
        eps, k = eps0, args[0]
    elif len(args) == 1:  # gomp(A,b,l,eps) with k = size(A,1) :126
        eps, k = args[0], M
    elif len(args) == 2:
        eps, k = args
    else:
        raise TypeError("gomp(A, b, l, [eps,] k)")
    _check_eps(eps)
    if int(l) < 1:
        raise ValueError("l has to be positive")
    D, tmp = _dict(A)
    try:
        idx, val, _ = D.ctx.gomp(b, int(l), int(k), float(eps))
        return SparseVector(N, idx, val)
    finally:
        if tmp:
            D.close()


def mp(A, b, k, x=None):
    """mp(A,b,k,x=spzeros(N)): k steps; x is a warm start and is updated in place like the reference."""
    D, tmp = _dict(A)
    try:
        M, N = D.shape
        i0 = v0 = None
        if x is not None and x.nnz:
            i0, v0 = x.nzind, x.nzval
        idx, val = D.ctx.mp(b, int(k), i0, v0)
        if x is None:
            return SparseVector(N, idx, val)
        x.nzind, x.nzval = idx, val
        return x
    finally:
        if tmp:
            D.close()


def shrinkage(x, a):
    """shrinkage(x, α) = sign(x) max(|x| - α, 0), the soft-thresholding operator (src/basispursuit.jl:144); scalars or arrays."""
    return np.sign(x) * np.maximum(np.abs(x) - a, 0.0)


def _ista(A, b, lam_or_w, x, maxiter, stepsize, accel):
    M, N, _ = _meta(A)
    w = np.atleast_1d(np.asarray(lam_or_w, dtype=np.float64))
    if w.ndim != 1 or len(w) not in (1, N):
        raise ValueError(f"length(w) = {w.shape} but size(A, 2) = {N}")  # DimensionMismatch("length(x) ≠ length(w)"), :155
    if not maxiter >= 0:
        raise ValueError(f"maxiter = {maxiter} has to be non-negative")
    if not (stepsize > 0 and np.isfinite(stepsize)):
        raise ValueError(f"stepsize = {stepsize} has to be positive and finite")
    D, tmp = _dict(A)
    try:
        i0 = v0 = None
        if x is not None and x.nnz:
            i0, v0 = x.nzind, x.nzval
        xd, _ = D.ctx.ista(b, w, i0, v0, maxiter=int(maxiter), stepsize=float(stepsize), accel=accel)
        nz = np.flatnonzero(xd)  # dropzeros!: an exact zero is a structural zero (:180)
        return SparseVector(N, nz, xd[nz])
    finally:
        if tmp:
            D.close()


def ista(A, b, lam_or_w, x=None, *, maxiter=1024, stepsize=1e-2):
    """ista(A,b,λ,x=spzeros(N); maxiter=1024, stepsize=1e-2) | ista(A,b,w,x; ...): exactly maxiter steps of
    x <- shrinkage(x + 2α A'(b - A x), wα) on ‖b - A x‖² + Σ w_j |x_j| (src/basispursuit.jl:164-183).  x is a warm start (not changed)."""
    return _ista(A, b, lam_or_w, x, maxiter, stepsize, False)


def fista(A, b, lam_or_w, x=None, *, maxiter=1024, stepsize=1e-2):
    """fista(A,b,λ | w,x; maxiter, stepsize): Beck-Teboulle acceleration of ista on the same objective -- t₁ = 1,
    t⁺ = (1 + √(1 + 4t²))/2, y⁺ = x⁺ + ((t - 1)/t⁺)(x⁺ - x).  The reference's own fista (:186-204) does not run."""
    return _ista(A, b, lam_or_w, x, maxiter, stepsize, True)


def _ista_batch(A, B, lam_or_w, X0, maxiter, stepsize, accel):
    M, N, _ = _meta(A)
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != M:
        raise ValueError(f"size(B) = {B.shape} but size(A, 1) = {M}: B holds one signal per column")
    nsig = B.shape[1]
    w, _, _ = _lib.ista_batch_weights(lam_or_w, N, nsig)
    if not np.all((w >= 0) & np.isfinite(w)):
        raise ValueError("the weights have to be non-negative and finite")
    if not maxiter >= 0:
        raise ValueError(f"maxiter = {maxiter} has to be non-negative")
    if not (stepsize > 0 and np.isfinite(stepsize)):
        raise ValueError(f"stepsize = {stepsize} has to be positive and finite")
    if X0 is not None:
        if isinstance(X0, (list, tuple)):
            if len(X0) != nsig or any(getattr(x, "n", None) != N for x in X0):
                raise ValueError(f"X0 has to hold {nsig} SparseVectors of length {N}")
            dense = np.zeros((N, nsig), np.float64, order="F")
            for s, x in enumerate(X0):
                dense[x.nzind, s] = x.nzval
            X0 = dense
        else:
            X0 = np.asarray(X0, dtype=np.float64)
            if X0.shape != (N, nsig):
                raise ValueError(f"size(X0) = {X0.shape} but the warm starts are size(A, 2) x nsig = {(N, nsig)}")
    D, tmp = _dict(A)
    try:
        X, _ = D.ctx.ista_batch(B, w, X0, maxiter=int(maxiter), stepsize=float(stepsize), accel=accel)
        xs = []
        for s in range(nsig):
            nz = np.flatnonzero(X[:, s])  # dropzeros!, as ista
            xs.append(SparseVector(N, nz, X[nz, s]))
        return xs
    finally:
        if tmp:
            D.close()


def ista_batch(A, B, lam_or_w, X0=None, *, maxiter=1024, stepsize=1e-2):
    """[ista(A, B[:, s], w_s, x0_s) for s in axes(B, 2)] on one GPU: up to eight signals take their iterations together, so the pass over
    the dictionary for A'r is read once per step for all of them.  Every result is ista's bit for bit.  lam_or_w: a scalar, an
    nsig-vector (one λ per signal: a regularisation path is the same b in every column), an N-vector (shared by all signals) or an
    N x nsig matrix (a weight vector per signal); when nsig == N a vector is the shared N-vector.  X0: the warm starts, a list of
    SparseVectors or a dense N x nsig matrix (not changed).  Returns a list of SparseVectors."""
    return _ista_batch(A, B, lam_or_w, X0, maxiter, stepsize, False)


def fista_batch(A, B, lam_or_w, X0=None, *, maxiter=1024, stepsize=1e-2):
    """[fista(A, B[:, s], w_s, x0_s) for s in axes(B, 2)]: ista_batch with fista's acceleration, every result fista's bit for bit."""
    return _ista_batch(A, B, lam_or_w, X0, maxiter, stepsize, True)


def _ista_joint(A, B, lam_or_w, X0, maxiter, stepsize, accel, return_info):
    M, N, _ = _meta(A)
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != M:
        raise ValueError(f"size(B) = {B.shape} but size(A, 1) = {M}: B holds one signal per column")
    nsig = B.shape[1]
    w = np.atleast_1d(np.asarray(lam_or_w, dtype=np.float64))
    if w.ndim != 1 or len(w) not in (1, N):
        raise ValueError(f"length(w) = {w.shape} but size(A, 2) = {N}: one weight, or one per row of X")
    if not np.all((w >= 0) & np.isfinite(w)):
        raise ValueError("the weights have to be non-negative and finite")
    if not maxiter >= 0:
        raise ValueError(f"maxiter = {maxiter} has to be non-negative")
    if not (stepsize > 0 and np.isfinite(stepsize)):
        raise ValueError(f"stepsize = {stepsize} has to be positive and finite")
    if X0 is not None:
        if isinstance(X0, (list, tuple)):
            if len(X0) != nsig or any(getattr(x, "n", None) != N for x in X0):
                raise ValueError(f"X0 has to hold {nsig} SparseVectors of length {N}")
            dense = np.zeros((N, nsig), np.float64, order="F")
            for s, x in enumerate(X0):
                dense[x.nzind, s] = x.nzval
            X0 = dense
        else:
            X0 = np.asarray(X0, dtype=np.float64)
            if X0.shape != (N, nsig):
                raise ValueError(f"size(X0) = {X0.shape} but the warm start is size(A, 2) x nsig = {(N, nsig)}")
    D, tmp = _dict(A)
    try:
        X, info = D.ctx.ista_joint(B, w, X0, maxiter=int(maxiter), stepsize=float(stepsize), accel=accel)
        nz = np.flatnonzero(np.any(X != 0, axis=1))  # the non-zero rows: ONE support (entries that are exactly zero stay in)
        xs = [SparseVector(N, nz.copy(), X[nz, s].copy()) for s in range(nsig)]
        return (xs, info) if return_info else xs
    finally:
        if tmp:
            D.close()


def ista_joint(A, B, lam_or_w, X0=None, *, maxiter=1024, stepsize=1e-2, return_info=False):
    """ista for columns of B that share ONE support: exactly maxiter steps of the proximal-gradient iteration on the row-sparse (l2,1)
    objective ‖B − A X‖_F² + Σ_j w_j ‖X[j, :]‖₂ -- U = X + 2α Aᵀ(B − A X), X⁺[j, :] = max(1 − w_j α / ‖U[j, :]‖₂, 0) U[j, :] (include/csmp.h,
    csmp_ista_joint).  The convex counterpart of somp; one column is ista.  lam_or_w: a scalar or an N-vector (one weight per ROW of X).
    X0: the warm start, a list of SparseVectors or a dense N x nsig matrix (not changed).  Returns a list of SparseVectors that all carry
    the same nzind (the non-zero rows); return_info=True: (xs, info) with rows (their number) and resnorm (‖b_l − A x_l‖ per column)."""
    return _ista_joint(A, B, lam_or_w, X0, maxiter, stepsize, False, return_info)


def fista_joint(A, B, lam_or_w, X0=None, *, maxiter=1024, stepsize=1e-2, return_info=False):
    """ista_joint with fista's acceleration: Y⁺ = X⁺ + ((t − 1)/t⁺)(X⁺ − X), t₁ = 1, the step taken from Y."""
    return _ista_joint(A, B, lam_or_w, X0, maxiter, stepsize, True, return_info)


# ------------------------------------------------------------------------------------ reweighted l1
def candes_weights(x, eps=1e-2):
    """candes_weights!(w, x, ε): w_j = 1 / (|x_j| + ε) (src/basispursuit.jl:33-39), Float64[N]; x a vector or a SparseVector.  NaN or Inf
    in the result is an error, as in the reference."""
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"eps = {eps} has to be positive and finite")
    x = x.to_dense() if isinstance(x, SparseVector) else np.asarray(x, dtype=np.float64)
    w = 1.0 / (np.abs(x) + eps)
    if not np.all(np.isfinite(w)):
        raise ValueError("weights contain NaN or Inf")
    return w


def ard_weights(A, x, w=None, eps=1e-2, iter=8):
    """ard_weights!(w, A, x, ε, iter) (src/basispursuit.jl:49-65): iter times over, d = |x| ./ w, K = εI + A diag(d) Aᵀ,
    w_j = √max(a_jᵀ K⁻¹ a_j, 0).  Returns the new weights, Float64[N]; w (default: ones) is not changed.  A zero weight is an error
    ("weights cannot be zero"); nnz(x) ≤ min(size(A, 1), 1024)."""
    M, N, _ = _meta(A)
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"eps = {eps} has to be positive and finite")
    if not _is_int(iter) or iter < 1:
        raise ValueError(f"iter = {iter} has to be at least 1")
    x = x.to_dense() if isinstance(x, SparseVector) else np.asarray(x, dtype=np.float64)
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    if x.shape != (N,) or w.shape != (N,):
        raise ValueError(f"length(x) = {x.shape}, length(w) = {w.shape} but size(A, 2) = {N}")
    if np.any(w == 0):
        raise ValueError("weights cannot be zero")
    D, tmp = _dict(A)
    try:
        return D.ctx.ard_weights(x, w, float(eps), int(iter))
    finally:
        if tmp:
            D.close()


def _ista_reweighted(A, b, lam, scheme, eps, maxiter, min_decrease, inner_maxiter, stepsize, accel, return_weights, ard_iter=8):
    M, N, _ = _meta(A)
    if not (lam >= 0 and np.isfinite(lam)):
        raise ValueError(f"lam = {lam} has to be non-negative and finite")
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"eps = {eps} has to be positive and finite")
    if not _is_int(maxiter) or maxiter < 1:
        raise ValueError(f"maxiter = {maxiter} has to be at least 1")
    if not min_decrease >= 0:
        raise ValueError(f"min_decrease = {min_decrease} has to be non-negative")
    if not inner_maxiter >= 0:
        raise ValueError(f"inner_maxiter = {inner_maxiter} has to be non-negative")
    if not (stepsize > 0 and np.isfinite(stepsize)):
        raise ValueError(f"stepsize = {stepsize} has to be positive and finite")
    D, tmp = _dict(A)
    try:
        out = D.ctx.ista_reweighted(b, float(lam), scheme, float(eps), ard_iter, int(maxiter), float(min_decrease), int(inner_maxiter),
                                    float(stepsize), accel, return_weights)
        nz = np.flatnonzero(out[0])
        x = SparseVector(N, nz, out[0][nz])
        return (x, out[3]) if return_weights else x
    finally:
        if tmp:
            D.close()


def ista_candes(A, b, lam, eps=1e-2, *, maxiter=8, min_decrease=1e-8, inner_maxiter=1024, stepsize=1e-2, accel=False, return_weights=False):
    """candes_reweighting (bp_candes, src/basispursuit.jl:18-45) with ista (accel=True: fista) as the solver of
    ‖b - A x‖² + λ Σ w_j |x_j|: x = solve(w = 1); up to maxiter - 1 times w_j = 1 / (|x_j| + ε), xs = solve(w) warm-started from x,
    stop once ‖xs - x‖ < min_decrease.  return_weights=True: (x, the last w)."""
    return _ista_reweighted(A, b, lam, "candes", eps, maxiter, min_decrease, inner_maxiter, stepsize, accel, return_weights)


def ista_ard(A, b, lam, eps=1e-2, *, maxiter=8, min_decrease=1e-8, inner_maxiter=1024, stepsize=1e-2, accel=False, return_weights=False, iter=8):
    """ard_reweighting (bp_ard, src/basispursuit.jl:18-31,49-74) with ista / fista as the solver: as ista_candes with
    ard_weights!(w, A, x, ε, iter) on the weights of the previous outer iteration (from ones)."""
    if not _is_int(iter) or iter < 1:
        raise ValueError(f"iter = {iter} has to be at least 1")
    return _ista_reweighted(A, b, lam, "ard", eps, maxiter, min_decrease, inner_maxiter, stepsize, accel, return_weights, int(iter))


# ------------------------------------------------------------------------------------ basis pursuit
def _bp_knobs(A, rho, maxiter, tol, check_every):
    M, N, _ = _meta(A)
    if M > N:
        raise ValueError(f"size(A) = {(M, N)}: A Aᵀ is singular when size(A, 1) > size(A, 2)")
    if not (rho > 0 and np.isfinite(rho)):
        raise ValueError(f"rho = {rho} has to be positive and finite")
    if not (tol > 0 and np.isfinite(tol)):
        raise ValueError(f"tol = {tol} has to be positive and finite")
    if not maxiter >= 0:
        raise ValueError(f"maxiter = {maxiter} has to be non-negative")
    if not _is_int(check_every) or check_every < 1:
        raise ValueError(f"check_every = {check_every} has to be at least 1")
    return M, N


def bp(A, b, w=None, *, rho=1.0, maxiter=16384, tol=1e-8, check_every=32, return_info=False):
    """bp(A, b[, w]) = basispursuit (src/basispursuit.jl:1-16): min Σ w_j |x_j| subject to A x = b, w = ones by default.  ADMM on the
    split x = z with one Cholesky factorisation of A Aᵀ per Dictionary (kept until its dictionary changes: M² + (2M)² doubles of
    device memory, 128 MiB + 512 MiB at M = 4096); every check_every iterations the primal and dual residuals are read, and the iteration
    stops once both are below tol.  Returns the exactly sparse z; return_info=True: (z, info) with info = {iterations, converged,
    factored, resnorm = ‖b − A z‖}.  Reaching maxiter is no error (converged is False).  A without full row rank is a ValueError."""
    M, N = _bp_knobs(A, rho, maxiter, tol, check_every)
    w = np.ones(1) if w is None else np.atleast_1d(np.asarray(w, dtype=np.float64))
    if w.ndim != 1 or len(w) not in (1, N):
        raise ValueError(f"length(w) = {w.shape} but size(A, 2) = {N}")
    if not np.all((w >= 0) & np.isfinite(w)):
        raise ValueError("the weights have to be non-negative and finite")
    D, tmp = _dict(A)
    try:
        try:
            xd, info = D.ctx.bp(b, w, float(rho), int(maxiter), float(tol), int(check_every))
        except CsmpError as e:
            if e.code == _lib.EINVAL and "positive definite" in str(e):
                raise ValueError(str(e)) from None
            raise
        nz = np.flatnonzero(xd)
        x = SparseVector(N, nz, xd[nz])
        return (x, info) if return_info else x
    finally:
        if tmp:
            D.close()


basispursuit = bp


def bp_batch(A, B, w=None, *, rho=1.0, maxiter=16384, tol=1e-8, check_every=32, return_info=False):
    """[bp(A, B[:, s], w) for s in axes(B, 2)] on one GPU: up to eight signals take their ADMM iterations in lockstep, so the dictionary,
    R⁻¹, R⁻ᵀ and G = A Aᵀ are read once per step for all of them; a finished signal's place is taken by the next column.  Every result is
    bp's bit for bit.  The weights are shared by all signals.  Returns a list of SparseVectors; return_info=True: (list, info) with
    info = {iterations int64[nsig], converged bool[nsig], resnorm float64[nsig], factored}."""
    M, N = _bp_knobs(A, rho, maxiter, tol, check_every)
    w = np.ones(1) if w is None else np.atleast_1d(np.asarray(w, dtype=np.float64))
    if w.ndim != 1 or len(w) not in (1, N):
        raise ValueError(f"length(w) = {w.shape} but size(A, 2) = {N}")
    if not np.all((w >= 0) & np.isfinite(w)):
        raise ValueError("the weights have to be non-negative and finite")
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != M:
        raise ValueError(f"size(B) = {B.shape} but size(A, 1) = {M}: B holds one signal per column")
    D, tmp = _dict(A)
    try:
        try:
            X, info = D.ctx.bp_batch(B, w, float(rho), int(maxiter), float(tol), int(check_every))
        except CsmpError as e:
            if e.code == _lib.EINVAL and "positive definite" in str(e):
                raise ValueError(str(e)) from None
            raise
        xs = []
        for s in range(X.shape[1]):
            nz = np.flatnonzero(X[:, s])
            xs.append(SparseVector(N, nz, X[nz, s]))
        return (xs, info) if return_info else xs
    finally:
        if tmp:
            D.close()


def bp_joint(A, B, w=None, *, rho=1.0, maxiter=16384, tol=1e-8, check_every=32, return_info=False):
    """bp for columns of B that share ONE support: min Σ_j w_j ‖X[j, :]‖₂ subject to A X = B, the row-sparse (l2,1, "MMV") programme --
    bp's ADMM with matrices in place of vectors and the shrinkage on whole rows, Z⁺[j, :] = max(1 − w_j / (ρ ‖T[j, :]‖₂), 0) T[j, :]
    (include/csmp.h, csmp_bp_joint).  No λ and no step size; the equality-constrained companion of ista_joint and the convex
    counterpart of somp; one column is bp.  ONE stopping rule for all columns: every check_every iterations ‖U⁺ − U‖_F and ρ‖Z⁺ − Z‖_F
    are read, and the iteration stops once both are below tol.  w: None (ones), a scalar or an N-vector (one weight per ROW of X).
    Returns a list of SparseVectors that all carry the same nzind (the non-zero rows); return_info=True: (xs, info) with
    info = {iterations, converged, factored, rows, resnorm (‖b_l − A x_l‖ per column)}.  Reaching maxiter is no error."""
    M, N = _bp_knobs(A, rho, maxiter, tol, check_every)
    w = np.ones(1) if w is None else np.atleast_1d(np.asarray(w, dtype=np.float64))
    if w.ndim != 1 or len(w) not in (1, N):
        raise ValueError(f"length(w) = {w.shape} but size(A, 2) = {N}: one weight, or one per row of X")
    if not np.all((w >= 0) & np.isfinite(w)):
        raise ValueError("the weights have to be non-negative and finite")
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != M:
        raise ValueError(f"size(B) = {B.shape} but size(A, 1) = {M}: B holds one signal per column")
    D, tmp = _dict(A)
    try:
        try:
            X, info = D.ctx.bp_joint(B, w, float(rho), int(maxiter), float(tol), int(check_every))
        except CsmpError as e:
            if e.code == _lib.EINVAL and "positive definite" in str(e):
                raise ValueError(str(e)) from None
            raise
        nz = np.flatnonzero(np.any(X != 0, axis=1))  # the non-zero rows: ONE support (entries that are exactly zero stay in)
        xs = [SparseVector(N, nz.copy(), X[nz, s].copy()) for s in range(X.shape[1])]
        return (xs, info) if return_info else xs
    finally:
        if tmp:
            D.close()


def _bp_reweighted(A, b, scheme, eps, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, return_weights, ard_iter=8):
    M, N = _bp_knobs(A, rho, inner_maxiter, tol, check_every)
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"eps = {eps} has to be positive and finite")
    if not _is_int(maxiter) or maxiter < 1:
        raise ValueError(f"maxiter = {maxiter} has to be at least 1")
    if not min_decrease >= 0:
        raise ValueError(f"min_decrease = {min_decrease} has to be non-negative")
    D, tmp = _dict(A)
    try:
        try:
            out = D.ctx.bp_reweighted(b, scheme, float(eps), ard_iter, int(maxiter), float(min_decrease), float(rho), int(inner_maxiter), float(tol),
                                      int(check_every), return_weights)
        except CsmpError as e:
            if e.code == _lib.EINVAL and "positive definite" in str(e):
                raise ValueError(str(e)) from None
            raise
        nz = np.flatnonzero(out[0])
        x = SparseVector(N, nz, out[0][nz])
        return (x, out[3]) if return_weights else x
    finally:
        if tmp:
            D.close()


def bp_candes(A, b, eps=1e-2, *, maxiter=8, min_decrease=1e-8, rho=1.0, inner_maxiter=16384, tol=1e-8, check_every=32, return_weights=False):
    """bp_candes(A, b, ε; maxiter, min_decrease) (src/basispursuit.jl:18-45): x = bp(A, b); up to maxiter − 1 times w_j = 1 / (|x_j| + ε),
    xs = bp(A, b, w) warm-started from the previous solve's iterates, stop once ‖xs − x‖ < min_decrease.  rho, inner_maxiter, tol,
    check_every: bp's, for every solve.  return_weights=True: (x, the last w)."""
    return _bp_reweighted(A, b, "candes", eps, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, return_weights)


def bp_ard(A, b, eps=1e-2, *, maxiter=8, min_decrease=1e-8, iter=8, rho=1.0, inner_maxiter=16384, tol=1e-8, check_every=32, return_weights=False):
    """bp_ard(A, b, ε; maxiter, min_decrease, iter) (src/basispursuit.jl:18-31,49-74): as bp_candes with ard_weights!(w, A, x, ε, iter)
    on the weights of the previous outer iteration (from ones); an iterate with more than min(size(A, 1), 1024) non-zeros is refused."""
    if not _is_int(iter) or iter < 1:
        raise ValueError(f"iter = {iter} has to be at least 1")
    return _bp_reweighted(A, b, "ard", eps, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, return_weights, int(iter))


# ------------------------------------------------------------------------------------ basis pursuit denoising
BPD_RHO = _lib.BPD_RHO  # the default penalty: the smallest total of the iteration table of DESIGN.md section 14


def _bpd_knobs(A, delta, rho, maxiter, tol, check_every):
    M, N, _ = _meta(A)
    if not (delta >= 0 and np.isfinite(delta)):
        raise ValueError(f"delta = {delta} has to be non-negative and finite")
    if not (rho > 0 and np.isfinite(rho)):
        raise ValueError(f"rho = {rho} has to be positive and finite")
    if not (tol > 0 and np.isfinite(tol)):
        raise ValueError(f"tol = {tol} has to be positive and finite")
    if not maxiter >= 0:
        raise ValueError(f"maxiter = {maxiter} has to be non-negative")
    if not _is_int(check_every) or check_every < 1:
        raise ValueError(f"check_every = {check_every} has to be at least 1")
    return M, N


def bpd(A, b, delta, w=None, *, rho=BPD_RHO, maxiter=16384, tol=1e-8, check_every=32, return_info=False):
    """bpd(A, b, δ[, w]) = basis_pursuit_denoising (src/basispursuit.jl:76-100): min Σ w_j |x_j| subject to ‖A x − b‖₂ ≤ δ, w = ones by
    default -- basis pursuit for data that carry noise.  Graph-form ADMM with one Cholesky factorisation of I + A Aᵀ per Dictionary (kept
    until its dictionary changes, apart from bp's factor: (2M)² doubles of device memory, 512 MiB at M = 4096); every check_every iterations
    the primal and dual residuals are read, and the iteration stops once both are below tol.  I + A Aᵀ is positive definite for every A:
    more rows than columns and rank-deficient dictionaries are served.  δ = 0 is bp's problem.  Returns the exactly sparse z;
    return_info=True: (z, info) with info = {iterations, converged, factored, resnorm = ‖b − A z‖}.  Reaching maxiter is no error
    (converged is False)."""
    M, N = _bpd_knobs(A, delta, rho, maxiter, tol, check_every)
    w = np.ones(1) if w is None else np.atleast_1d(np.asarray(w, dtype=np.float64))
    if w.ndim != 1 or len(w) not in (1, N):
        raise ValueError(f"length(w) = {w.shape} but size(A, 2) = {N}")
    if not np.all((w >= 0) & np.isfinite(w)):
        raise ValueError("the weights have to be non-negative and finite")
    D, tmp = _dict(A)
    try:
        xd, info = D.ctx.bpd(b, float(delta), w, float(rho), int(maxiter), float(tol), int(check_every))
        nz = np.flatnonzero(xd)
        x = SparseVector(N, nz, xd[nz])
        return (x, info) if return_info else x
    finally:
        if tmp:
            D.close()


basis_pursuit_denoising = bpd


def bpd_batch(A, B, delta, w=None, *, rho=BPD_RHO, maxiter=16384, tol=1e-8, check_every=32, return_info=False):
    """[bpd(A, B[:, s], δ[s], w) for s in axes(B, 2)] on one GPU: up to eight signals take their ADMM iterations in lockstep, so the
    dictionary and the two triangular factors of I + A Aᵀ are read once per step for all of them; a finished signal's place is taken by the
    next column.  Every result is bpd's bit for bit.  δ: a scalar, or a 1-D array with one radius per column of B; the weights are shared
    by all signals.  Returns a list of SparseVectors; return_info=True: (list, info) with info = {iterations int64[nsig], converged
    bool[nsig], resnorm float64[nsig], factored}."""
    M, N = _bpd_knobs(A, 0.0, rho, maxiter, tol, check_every)
    w = np.ones(1) if w is None else np.atleast_1d(np.asarray(w, dtype=np.float64))
    if w.ndim != 1 or len(w) not in (1, N):
        raise ValueError(f"length(w) = {w.shape} but size(A, 2) = {N}")
    if not np.all((w >= 0) & np.isfinite(w)):
        raise ValueError("the weights have to be non-negative and finite")
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != M:
        raise ValueError(f"size(B) = {B.shape} but size(A, 1) = {M}: B holds one signal per column")
    delta = np.asarray(delta, dtype=np.float64)
    if delta.ndim > 1 or (delta.ndim == 1 and len(delta) != B.shape[1]):
        raise ValueError(f"size(delta) = {delta.shape} but B has {B.shape[1]} columns: a scalar, or one radius per signal")
    delta = np.atleast_1d(delta)
    if not np.all((delta >= 0) & np.isfinite(delta)):
        raise ValueError("every delta has to be non-negative and finite")
    D, tmp = _dict(A)
    try:
        X, info = D.ctx.bpd_batch(B, delta, w, float(rho), int(maxiter), float(tol), int(check_every))
        xs = []
        for s in range(X.shape[1]):
            nz = np.flatnonzero(X[:, s])
            xs.append(SparseVector(N, nz, X[nz, s]))
        return (xs, info) if return_info else xs
    finally:
        if tmp:
            D.close()


def _bpd_reweighted(A, b, delta, scheme, eps, maxiter, min_decrease, rho, inner_maxiter, tol, check_every, return_weights, ard_iter=8):
    M, N = _bpd_knobs(A, delta, rho, inner_maxiter, tol, check_every)
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"eps = {eps} has to be positive and finite")
    if not _is_int(maxiter) or maxiter < 1:
        raise ValueError(f"maxiter = {maxiter} has to be at least 1")
    if not min_decrease >= 0:
        raise ValueError(f"min_decrease = {min_decrease} has to be non-negative")
    D, tmp = _dict(A)
    try:
        out = D.ctx.bpd_reweighted(b, float(delta), scheme, float(eps), ard_iter, int(maxiter), float(min_decrease), float(rho), int(inner_maxiter),
                                   float(tol), int(check_every), return_weights)
        nz = np.flatnonzero(out[0])
        x = SparseVector(N, nz, out[0][nz])
        return (x, out[3]) if return_weights else x
    finally:
        if tmp:
            D.close()


def bpd_candes(A, b, delta, eps=None, *, maxiter=8, min_decrease=1e-4, rho=BPD_RHO, inner_maxiter=16384, tol=1e-8, check_every=32,
               return_weights=False):
    """bpd_candes(A, b, δ, ε = δ; maxiter) (src/basispursuit.jl:102-121): x = bpd(A, b, δ); up to maxiter − 1 times w_j = 1 / (|x_j| + ε),
    xs = bpd(A, b, δ, w) warm-started from the previous solve's iterates, stop once ‖xs − x‖ < min_decrease.  rho, inner_maxiter, tol,
    check_every: bpd's, for every solve.  return_weights=True: (x, the last w)."""
    return _bpd_reweighted(A, b, delta, "candes", delta if eps is None else eps, maxiter, min_decrease, rho, inner_maxiter, tol, check_every,
                           return_weights)


def bpd_ard(A, b, delta, eps=None, *, maxiter=8, min_decrease=1e-4, iter=8, rho=BPD_RHO, inner_maxiter=16384, tol=1e-8, check_every=32,
            return_weights=False):
    """bpd_ard(A, b, δ, ε = δ²; maxiter, iter) (src/basispursuit.jl:102-115,122-124): as bpd_candes with ard_weights!(w, A, x, ε, iter) on
    the weights of the previous outer iteration (from ones); an iterate with more than min(size(A, 1), 1024) non-zeros is refused."""
    if not _is_int(iter) or iter < 1:
        raise ValueError(f"iter = {iter} has to be at least 1")
    return _bpd_reweighted(A, b, delta, "ard", delta ** 2 if eps is None else eps, maxiter, min_decrease, rho, inner_maxiter, tol, check_every,
                           return_weights, int(iter))


# ------------------------------------------------------------------------------------ sparse Bayesian learning
def _sbl_knobs(A, b, sigma2, maxiter, min_change):
    M, N, _ = _meta(A)
    if np.ndim(sigma2) != 0:
        raise NotImplementedError("sbl: a noise covariance matrix Σ is not served: scalar σ² only")
    if not (sigma2 > 0 and np.isfinite(sigma2)):
        raise ValueError(f"σ² = {sigma2} has to be positive and finite")
    if not min_change >= 0:
        raise ValueError(f"min_change = {min_change} has to be non-negative")
    if maxiter is not None and (not _is_int(maxiter) or maxiter < 1):
        raise ValueError(f"maxiter = {maxiter} has to be at least 1")
    if np.shape(b) != (M,):
        raise ValueError(f"DimensionMismatch: size(A, 1) = {M} != {np.shape(b)} = size(b)")
    return M, N


def sbl(A, b, sigma2, *, maxiter=None, min_change=1e-6, return_info=False):
    """sbl(A, b, σ²; maxiter = 128 size(A, 2), min_change = 1e-6) (src/sbl.jl:37-51): sparse Bayesian learning for a scalar noise variance.
    From γ = 1, update!(::SBL) (:26-35) until ‖γ_old − γ‖ < min_change or maxiter updates are done; returns the DENSE x of the last update,
    Float64[N], as the reference does (its entries off the support are tiny, not zero).  Every update runs in the Woodbury form on the
    M × M matrix σ² I + A Γ Aᵀ (include/csmp.h, csmp_sbl) -- the reference's N × N factorisation is never formed -- so more rows than
    columns are served.  return_info=True: (x, info) with info = {iterations, converged, gamma}.  Reaching maxiter is no error
    (converged is False).  A noise covariance matrix raises NotImplementedError; fsbl and rmps are the greedy forms, below."""
    M, N = _sbl_knobs(A, b, sigma2, maxiter, min_change)
    D, tmp = _dict(A)
    try:
        x, info, gamma = D.ctx.sbl(b, float(sigma2), maxiter, float(min_change), return_gamma=True)
        info["gamma"] = gamma
        return (x, info) if return_info else x
    finally:
        if tmp:
            D.close()


# ------------------------------------------------------------------------------------ greedy sparse Bayesian learning
def _fsbl_knobs(who, A, b, sigma2, caps, min_increase, alpha):
    M, N, _ = _meta(A)
    if isinstance(sigma2, (bool, np.bool_)):  # the reference's rmps(A, b, Val(true), ...)
        raise NotImplementedError(f"{who}: the σ²-optimising form (Val(true)) is not served: pass the scalar noise variance σ²")
    if np.ndim(sigma2) != 0:
        raise NotImplementedError(f"{who}: only a scalar noise variance σ² is served, not a covariance matrix Σ")
    if not (sigma2 > 0 and np.isfinite(sigma2)):
        raise ValueError(f"σ² = {sigma2} has to be positive and finite")
    if not min_increase >= 0:
        raise ValueError(f"min_increase = {min_increase} has to be non-negative")
    for name, c in caps.items():
        if c is not None and (not _is_int(c) or c < 1):
            raise ValueError(f"{name} = {c} has to be at least 1")
    if np.shape(b) != (M,):
        raise ValueError(f"DimensionMismatch: size(A, 1) = {M} != {np.shape(b)} = size(b)")
    if alpha is not None:
        alpha = np.asarray(alpha, dtype=np.float64)
        if alpha.shape != (N,) or not np.all(alpha > 0):
            raise ValueError("every entry of alpha has to be positive, or +inf for an inactive atom")
    return M, N


def fsbl(A, b, sigma2, *, maxiter=None, min_increase=1e-6, alpha=None, return_info=False):
    """fsbl(A, b, σ²; maxiter = 2 size(A, 2), min_increase = 1e-6) (src/sbl.jl:149-176): fast sparse Bayesian learning for a scalar noise
    variance.  Every pass changes the prior precision α_i of the ONE atom whose addition, deletion or re-estimation raises the marginal
    likelihood most; the loop stops after the pass in which that increase is below min_increase, at the latest after maxiter passes
    (converged is then False; no error).  Returns x, Float64[N]: exactly 0 off the active set, Q_j / α_j on it -- the reference's solve
    (A_aᵀA_a/σ² + diag α_a) x_a = A_aᵀb/σ² in exact arithmetic (include/csmp.h, csmp_fsbl).  alpha: prior precisions to start from
    (+inf: inactive).  return_info=True: (x, info) with info = {iterations, converged, alpha, history}; history lists the applied steps
    as (action, index), 1 add, 2 delete, 3 re-estimate.  A noise covariance matrix raises NotImplementedError."""
    _fsbl_knobs("fsbl", A, b, sigma2, {"maxiter": maxiter}, min_increase, alpha)
    D, tmp = _dict(A)
    try:
        x, info = D.ctx.fsbl(b, float(sigma2), maxiter, float(min_increase), alpha)
        return (x, info) if return_info else x
    finally:
        if tmp:
            D.close()


def rmps(A, b, sigma2, *, maxiter=None, maxiter_acquisition=None, maxiter_deletion=None, min_increase=1e-6, alpha=None, return_info=False):
    """rmps(A, b, σ²; maxiter, maxiter_acquisition, maxiter_deletion = size(A, 1), min_increase = 1e-6) (src/sbl.jl:373-437): relevance
    matching pursuit for a scalar noise variance.  An outer iteration adds atoms while an addition raises the marginal likelihood, then
    deletes the active atom of least q²/s while that is below 1 and otherwise re-estimates the α_i that gains most, until that gain is
    below min_increase; it ends when α no longer changes.  x, alpha, return_info: as fsbl; info["iterations"] counts the applied steps.
    A noise covariance matrix and the σ²-optimising form (σ² = True, the reference's Val(true)) raise NotImplementedError."""
    _fsbl_knobs("rmps", A, b, sigma2, {"maxiter": maxiter, "maxiter_acquisition": maxiter_acquisition, "maxiter_deletion": maxiter_deletion},
                min_increase, alpha)
    D, tmp = _dict(A)
    try:
        x, info = D.ctx.rmps(b, float(sigma2), maxiter, maxiter_acquisition, maxiter_deletion, float(min_increase), alpha)
        return (x, info) if return_info else x
    finally:
        if tmp:
            D.close()


def _fsbl_batch(who, A, B, sigma2, caps, min_increase, alpha, return_info):
    M, N, _ = _meta(A)
    if isinstance(sigma2, (bool, np.bool_)):  # the reference's rmps(A, b, Val(true), ...)
        raise NotImplementedError(f"{who}: the σ²-optimising form (Val(true)) is not served: pass the noise variance σ²")
    if np.ndim(sigma2) > 1:
        raise NotImplementedError(f"{who}: only scalar noise variances σ² are served (one, or one per signal), not a covariance matrix Σ")
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != M:
        raise ValueError(f"size(B) = {B.shape} but size(A, 1) = {M}: B holds one signal per column")
    nsig = B.shape[1]
    s2 = np.asarray(sigma2, dtype=np.float64)
    if s2.ndim == 1 and s2.shape[0] != nsig:
        raise ValueError(f"length(σ²) = {s2.shape[0]} but B holds {nsig} signals")
    if not np.all((s2 > 0) & np.isfinite(s2)):
        raise ValueError(f"σ² = {sigma2} has to be positive and finite")
    if not min_increase >= 0:
        raise ValueError(f"min_increase = {min_increase} has to be non-negative")
    for name, c in caps.items():
        if c is not None and (not _is_int(c) or c < 1):
            raise ValueError(f"{name} = {c} has to be at least 1")
    if alpha is not None:
        alpha = np.asarray(alpha, dtype=np.float64)
        if alpha.shape != (N, nsig) or not np.all(alpha > 0):
            raise ValueError("alpha has to be size(A, 2) x nsig with every entry positive, or +inf for an inactive atom")
    D, tmp = _dict(A)
    try:
        X, info = getattr(D.ctx, who)(B, s2, *caps.values(), float(min_increase), alpha)
        xs = []
        for s in range(nsig):
            nz = np.flatnonzero(X[:, s])
            xs.append(SparseVector(N, nz, X[nz, s]))
        return (xs, info) if return_info else xs
    finally:
        if tmp:
            D.close()


def fsbl_batch(A, B, sigma2, *, maxiter=None, min_increase=1e-6, alpha=None, return_info=False):
    """[fsbl(A, B[:, s], σ²_s) for s in axes(B, 2)] on one GPU: up to eight signals take their greedy steps in lockstep, so the product
    sweep of a step reads the dictionary once for all of them (include/csmp.h, csmp_fsbl_batch).  Every result is fsbl's bit for bit.
    sigma2: one noise variance, or one per signal.  alpha: None, or the N x nsig prior precisions to start from (+inf: inactive).
    Returns a list of SparseVectors; return_info=True: (xs, info) with the per-signal iterations, converged, alpha (N x nsig) and
    history.  A noise covariance matrix raises NotImplementedError."""
    return _fsbl_batch("fsbl_batch", A, B, sigma2, {"maxiter": maxiter}, min_increase, alpha, return_info)


def rmps_batch(A, B, sigma2, *, maxiter=None, maxiter_acquisition=None, maxiter_deletion=None, min_increase=1e-6, alpha=None,
               return_info=False):
    """[rmps(A, B[:, s], σ²_s) for s in axes(B, 2)] on one GPU: as fsbl_batch, every result rmps's bit for bit.  A noise covariance matrix
    and the σ²-optimising form (σ² = True) raise NotImplementedError."""
    return _fsbl_batch("rmps_batch", A, B, sigma2, {"maxiter": maxiter, "maxiter_acquisition": maxiter_acquisition,
                                                    "maxiter_deletion": maxiter_deletion}, min_increase, alpha, return_info)


# ------------------------------------------------------------------------------------ dictionary analysis
def colnorms(A):
    """colnorms(A) = [norm(a) for a in eachcol(A)] (src/util.jl:2), Float64."""
    D, tmp = _dict(A)
    try:
        return D.ctx.colnorms()
    finally:
        if tmp:
            D.close()


def _cumbabel(A, k, normalize):
    _, N, _ = _meta(A)
    if not _is_int(k) or not 1 <= k <= min(N, _lib.BABEL_KMAX):
        raise ValueError(f"k = {k} has to lie in 1 .. min(size(A, 2), {_lib.BABEL_KMAX}) = {min(N, _lib.BABEL_KMAX)}")
    if normalize not in (False, True, 0, 1):
        raise ValueError(f"normalize = {normalize} has to be False or True")
    D, tmp = _dict(A)
    try:
        return D.ctx.cumbabel(int(k), bool(normalize))
    finally:
        if tmp:
            D.close()


def cumbabel(A, k, normalize=False):
    """cumbabel(A, k): the Babel function μ₁(1..k) (src/util.jl:103-115) -- for every column the k largest |⟨a_i, a_j⟩|, j ≠ i, in
    descending order, their running sums, the maximum over the columns.  The inner products are raw, as in the reference (which
    assumes unit-norm columns); normalize=True divides each by ‖a_i‖ ‖a_j‖ (a zero column contributes 0).  k ≤ min(N, 1024)."""
    return _cumbabel(A, k, normalize)[0]


def babel(A, k, normalize=False):
    """babel(A, k) = cumbabel(A, k)[k] (src/util.jl:99)."""
    return float(_cumbabel(A, k, normalize)[0][-1])


def coherence(A, normalize=False, return_pair=False):
    """coherence(A) = babel(A, 1) (src/util.jl:96), the mutual coherence.  return_pair=True: (μ, (i, j)) with the 0-based columns
    i < j that attain it (the lowest i, then the lowest j among equals; (-1, -1) for a single column)."""
    mu, pair = _cumbabel(A, 1, normalize)
    return (float(mu[0]), pair) if return_pair else float(mu[0])


def sp(A, b, k, delta=1e-12, maxiter=None):
    """sp(A,b,k,delta=1e-12; maxiter=16k).  2k > length(b) is an error (src/twostage.jl:55)."""
    M, N, _ = _meta(A)
    if 2 * k > M:
        raise ValueError(f"2k = {2 * k} > {M} = length(b) is invalid for Subspace Pursuit")
    D, tmp = _dict(A)
    try:
        idx, val, _ = D.ctx.sp(b, int(k), float(delta), -1 if maxiter is None else int(maxiter))
        return SparseVector(N, idx, val)
    finally:
        if tmp:
            D.close()


def ompr(A, b, k, delta, maxiter=None):
    """ompr(A,b,k,delta; maxiter=size(A,1)): OMP with replacement, src/twostage.jl:184-202 (x empty)."""
    D, tmp = _dict(A)
    try:
        idx, val, _ = D.ctx.ompr(b, int(k), float(delta), -1 if maxiter is None else int(maxiter))
        return SparseVector(D.shape[1], idx, val)
    finally:
        if tmp:
            D.close()


def ompr_batch(A, B, k, delta, maxiter=None, return_info=False):
    """[ompr(A, B[:, s], k, delta_s; maxiter) for s in axes(B, 2)] on one GPU: up to eight signals take their update! in lockstep, so the
    product sweep of an iteration reads the dictionary once for all of them (include/csmp.h, csmp_ompr_batch).  Every result is ompr's
    bit for bit.  delta: one threshold, or one per column.  Returns a list of SparseVectors; return_info=True: (xs, info) with the
    per-signal iterations and solved_alone (the signal left its group and was solved by the single path)."""
    M, N, _ = _meta(A)
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != M:
        raise ValueError(f"size(B) = {B.shape} but size(A, 1) = {M}: B holds one signal per column")
    nsig = B.shape[1]
    if not _is_int(k) or not 1 <= k <= min(M, N):
        raise ValueError(f"k = {k} has to lie in 1 .. min(size(A)) = {min(M, N)}")
    d = np.asarray(delta, dtype=np.float64)
    if d.ndim > 1 or (d.ndim == 1 and d.shape[0] != nsig):
        raise ValueError(f"delta has to be a scalar or one value per signal: size(delta) = {d.shape} but B holds {nsig} signals")
    if np.any(np.isnan(d)):
        raise ValueError(f"delta = {delta} is NaN")
    if maxiter is not None and (not _is_int(maxiter) or maxiter < 0):
        raise ValueError(f"maxiter = {maxiter} has to be a non-negative integer")
    D, tmp = _dict(A)
    try:
        idx, val, nnz, info = D.ctx.ompr_batch(B, int(k), d, maxiter)
        xs = [SparseVector(N, idx[:nnz[s], s].copy(), val[:nnz[s], s].copy()) for s in range(nsig)]
        return (xs, info) if return_info else xs
    finally:
        if tmp:
            D.close()


def fr(A, b, *args, max_residual=0.0, min_decrease=0.0, sparsity=None):
    """fr(A,b,max_eps,min_delta,k=size(A,1)) and fr(A,b; max_residual=0, min_decrease=0, sparsity=size(A,2)):
    forward regression / orthogonal least squares (src/forward.jl:34-54), x starting empty."""
    M, N, _ = _meta(A)
    if len(args) == 0:  # keyword form :34-37
        max_eps, min_delta, k = max_residual, min_decrease, (N if sparsity is None else sparsity)
    elif len(args) in (2, 3):
        max_eps, min_delta = args[0], args[1]
        k = args[2] if len(args) == 3 else M  # :45
    else:
        raise TypeError("fr(A, b, max_eps, min_delta[, k]) or fr(A, b; max_residual, min_decrease, sparsity)")
    if np.shape(b)[0] != M:  # FR(A, b): DimensionMismatch (:22)
        raise ValueError(f"DimensionMismatch: size(A, 1) = {M} != {np.shape(b)[0]} = length(b)")
    D, tmp = _dict(A)
    try:
        idx, val, _ = D.ctx.fr(b, min(int(k), M), float(max_eps), float(min_delta))
        return SparseVector(N, idx, val)
    finally:
        if tmp:
            D.close()


ols = oomp = ormp = fr  # src/forward.jl:52-54


def srr(A, b, k, delta=1e-12, maxiter=None, initialization=1, l=1, rng=None, init=None):
    """srr(A,b,k,delta=1e-12; maxiter=4k, initialization=1, l=1): stepwise regression with replacement,
    src/twostage.jl:3-33 (x empty).  initialization 3 = random_acquisition! (src/matchingpursuit.jl:195-204): the k initial
    atoms are drawn HERE, without replacement, from `rng` (a numpy Generator or a seed) -- the reference draws them from Julia's
    global RNG, so only the distribution matches, not the draw; pass `init` (k atom indices) to fix the draw itself."""
    D, tmp = _dict(A)
    try:
        if int(initialization) == 3 and init is None:
            init = np.random.default_rng(rng).choice(D.shape[1], size=int(k), replace=False)
        idx, val, _ = D.ctx.srr(b, int(k), float(delta), -1 if maxiter is None else int(maxiter), int(initialization), int(l), init)
        return SparseVector(D.shape[1], idx, val)
    finally:
        if tmp:
            D.close()


def rmp(A, b, delta_or_k, maxiter=1, kmax=None):
    """rmp(A, b, δ, maxiter=1) -- δ a float -- and rmp(A, b, k) -- k an int: relevance matching pursuit,
    src/stepwise.jl:5-43 (x empty).  kmax bounds the support of the forward stage (default min(M, N, 4095))."""
    D, tmp = _dict(A)
    try:
        idx, val = D.ctx.rmp(b, delta_or_k, maxiter, kmax)
        return SparseVector(D.shape[1], idx, val)
    finally:
        if tmp:
            D.close()


def foba(A, b, delta, kmax=None, isfast=True):
    """foba(A, b, δ; isfast): adaptive forward-backward greedy algorithm, src/stepwise.jl:47-56 (x empty).
    `isfast` is accepted for signature parity and has no effect: the reference's isfast = Val(false) computes the SAME
    backward scores |r_{-i}|^2 - |r|^2 by re-factorising without each column in turn (naive_backward_δ!, src/backward.jl:87-105)
    instead of x_i^2 / γ_i (backward_δ!, :79-83) -- one quantity, two costs; the device evaluates the closed form."""
    del isfast
    D, tmp = _dict(A)
    try:
        idx, val = D.ctx.foba(b, float(delta), kmax)
        return SparseVector(D.shape[1], idx, val)
    finally:
        if tmp:
            D.close()


def _backward(A, b, args, max_residual, max_increase, sparsity, lace, name):
    if len(args) == 0:  # keyword form (src/backward.jl:38-41,150-153,228-231)
        max_eps, max_delta, k = max_residual, max_increase, sparsity
    elif len(args) == 3:
        max_eps, max_delta, k = args
    else:
        raise TypeError(f"{name}(A, b, max_eps, max_delta, k) or {name}(A, b; max_residual, max_increase, sparsity)")
    M, N, _ = _meta(A)
    if N > M:
        raise ValueError(f"A needs to be overdetermined but is of size ({M}, {N})")  # :218
    D, tmp = _dict(A)
    try:
        idx, val = D.ctx.br(b, float(max_eps), float(max_delta), int(k), lace)
        return SparseVector(N, idx, val)
    finally:
        if tmp:
            D.close()


def br(A, b, *args, max_residual=float("inf"), max_increase=float("inf"), sparsity=0):
    """br(A,b,max_eps,max_delta,k) / br(A,b; max_residual=Inf, max_increase=Inf, sparsity=0): backward regression,
    src/backward.jl:27-41 (the default isfast = true scores)."""
    return _backward(A, b, args, max_residual, max_increase, sparsity, False, "br")


def fbr(A, b, *args, max_residual=float("inf"), max_increase=float("inf"), sparsity=0):
    """fbr: the same algorithm as br on the normal equations (src/backward.jl:148-162); here they share one path."""
    return _backward(A, b, args, max_residual, max_increase, sparsity, False, "fbr")


def lace(A, b, *args, max_residual=float("inf"), max_increase=float("inf"), sparsity=0):
    """lace(A,b,eps,delta,k): least absolute coefficient elimination, src/backward.jl:226-270."""
    return _backward(A, b, args, max_residual, max_increase, sparsity, True, "lace")


def omp_batch(A, B, k, eps=None):
    """[omp(A, B[:, s], eps, k) for s in axes(B, 2)] on one GPU; returns a list of SparseVectors."""
    eps = _meta(A)[2] if eps is None else eps
    _check_eps(eps)
    D, tmp = _dict(A)
    try:
        idx, val, nnz = D.ctx.omp_batch(B, int(k), float(eps))
        return [SparseVector(D.shape[1], idx[:n, s], val[:n, s]) for s, n in enumerate(nnz)]
    finally:
        if tmp:
            D.close()


def mp_batch(A, B, k):
    """[mp(A, B[:, s], k) for s in axes(B, 2)] on one GPU, x starting from 0 (up to eight signals share each pass over the dictionary):
    list of SparseVectors.  Warm starts stay with mp."""
    D, tmp = _dict(A)
    try:
        idx, val, nnz = D.ctx.mp_batch(B, int(k))
        return [SparseVector(D.shape[1], idx[:n, s].copy(), val[:n, s].copy()) for s, n in enumerate(nnz)]
    finally:
        if tmp:
            D.close()


def somp(A, B, *args, max_residual=None, sparsity=None, p=1, return_info=False):
    """somp(A,B,k) | somp(A,B,eps[,k]) | somp(A,B; max_residual=eps(T), sparsity=min(size(A)...), p=1): simultaneous OMP (Tropp, Gilbert
    and Strauss 2006) for columns of B that share ONE support -- omp's driver with the residual matrix in place of the residual: a step
    takes the atom that maximises sum_l |<a_j, r_l>|^p (p = 1 or 2), appends it to one factorisation and projects every residual; it ends
    after k atoms or once ||R||_F < eps (include/csmp.h, csmp_somp).  One column is omp.  Returns a list of SparseVectors that all carry
    the same nzind (entries that are exactly zero stay in); return_info=True: (xs, info) with order (the atoms as they were picked),
    resnorm (||r_l|| per column), steps and passes (the passes over the dictionary)."""
    M, N, eps0 = _meta(A)
    if len(args) == 0:
        eps = eps0 if max_residual is None else max_residual
        k = min(M, N) if sparsity is None else sparsity
    elif len(args) == 1 and _is_int(args[0]):
        eps, k = eps0, args[0]
    elif len(args) == 1:
        eps, k = args[0], min(M, N)
    elif len(args) == 2:
        eps, k = args
    else:
        raise TypeError("somp(A, B, [eps,] k)")
    _check_eps(eps)
    if not _is_int(k) or not 1 <= k <= min(M, N):
        raise ValueError(f"k = {k} has to lie in 1 .. min(size(A)) = {min(M, N)}")
    if not _is_int(p) or p not in (1, 2):
        raise ValueError(f"p = {p} has to be 1 or 2")
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != M:
        raise ValueError(f"size(B) = {B.shape} but size(A, 1) = {M}: B holds one signal per column")
    D, tmp = _dict(A)
    try:
        idx, val, info = D.ctx.somp(B, int(k), float(eps), int(p))
        xs = [SparseVector(N, idx.copy(), val[:, s].copy()) for s in range(B.shape[1])]
        return (xs, info) if return_info else xs
    finally:
        if tmp:
            D.close()


def gomp_batch(A, B, l, k, eps=None):
    """[gomp(A, B[:, s], l, eps, k) for s in axes(B, 2)] on one GPU (two solves in flight): list of SparseVectors."""
    eps = _meta(A)[2] if eps is None else eps
    _check_eps(eps)
    D, tmp = _dict(A)
    try:
        idx, val, nnz = D.ctx.gomp_batch(B, int(l), int(k), float(eps))
        return [SparseVector(D.shape[1], idx[:n, s], val[:n, s]) for s, n in enumerate(nnz)]
    finally:
        if tmp:
            D.close()


def sp_batch(A, B, k, delta=1e-12, maxiter=None):
    """[sp(A, B[:, s], k, delta; maxiter) for s in axes(B, 2)] on one GPU (several solves in flight): list of SparseVectors."""
    D, tmp = _dict(A)
    try:
        idx, val, nnz, its = D.ctx.sp_batch(B, int(k), float(delta), -1 if maxiter is None else int(maxiter))
        return [SparseVector(D.shape[1], idx[:n, s], val[:n, s]) for s, n in enumerate(nnz)]
    finally:
        if tmp:
            D.close()


def solve_in_flight(A, signals, solve, in_flight=3):
    """Any single-signal driver for many signals with `in_flight` solves at once on ONE GPU: `solve(ctx, b)` is called with a
    context of its own (the Dictionary's and `in_flight - 1` clones: own stream, own solver state, the same resident dictionary)
    from a host thread of its own -- the library calls release the GIL -- so that one signal's short, latency-bound stages run
    under another signal's dictionary sweeps (what csmp_gomp_batch / csmp_sp_batch do inside the library).  Returns the list
    of `solve`'s results in signal order.  Example: solve_in_flight(D, cols, lambda c, b: c.ompr(b, 64, 1e-6))."""
    import threading
    D, tmp = _dict(A)
    signals = list(signals)
    T = max(1, min(int(in_flight), len(signals)))
    ctxs = [D.ctx] + [D.ctx.clone() for _ in range(T - 1)]
    out = [None] * len(signals)
    err = [None] * T

    def work(t):
        try:
            for s in range(t, len(signals), T):
                out[s] = solve(ctxs[t], signals[s])
        except Exception as e:  # noqa: BLE001
            err[t] = e
    th = [threading.Thread(target=work, args=(t,)) for t in range(1, T)]
    try:
        for x in th:
            x.start()
        work(0)
    finally:
        for x in th:  # (also when work(0) left through a BaseException: no clone is closed under a thread that still uses it)
            if x.is_alive():
                x.join()
        for c in ctxs[1:]:
            c.close()
        if tmp:
            D.close()
    for e in err:
        if e is not None:
            raise e
    return out


def fr_batch(A, B, k, max_eps=0.0, min_delta=0.0):
    """[fr(A, B[:, s], max_eps, min_delta, k) for s in axes(B, 2)]: list of SparseVectors (pipelined on the device)."""
    D, tmp = _dict(A)
    try:
        idx, val, nnz = D.ctx.fr_batch(B, int(k), float(max_eps), float(min_delta))
        return [SparseVector(D.shape[1], idx[:nnz[s], s].copy(), val[:nnz[s], s].copy()) for s in range(idx.shape[1])]
    finally:
        if tmp:
            D.close()


def omp_batch_mfma(A, B, k, eps=None, cert=None, gram=None):
    """omp_batch through the batched variant (BASELINE configs 3/4): one bf16 MFMA screening GEMM per step for all
    signals, Float64 rescoring of the screened atoms that could still be the exact maximum, and a per-step certificate;
    signals that fail it are re-solved by the exact path, so certified results equal omp_batch's.
    cert: "rigorous" (the library's default: a deterministic error bound, a passed certificate proves the pick) or "statistical"
    (opt-in: 8 sigma of independent roundings + a coherent term; narrower windows, faster, NOT a proof -- see
    tests/test_gpu_parity.py::test_batched_certificate_against_adversarial_residuals); gram: True keeps G = A'A resident on the
    GPU (8 N^2 bytes) and halves the append traffic (csmp_set_option CSMP_OPT_BATCH_CERT / CSMP_OPT_BATCH_GRAM, include/csmp.h).
    Options given here hold for this call only: a caller-owned Dictionary gets its own values back."""
    eps = _meta(A)[2] if eps is None else eps
    _check_eps(eps)
    D, tmp = _dict(A)
    saved = {}
    try:
        if cert is not None:
            saved["batch_cert"] = D.ctx.get_option("batch_cert")
            D.ctx.set_option("batch_cert", {"statistical": 0, "rigorous": 1}[cert])
        if gram is not None:
            saved["batch_gram"] = D.ctx.get_option("batch_gram")
            D.ctx.set_option("batch_gram", int(bool(gram)))
        idx, val, nnz = D.ctx.omp_batch_mfma(B, int(k), float(eps))
        return [SparseVector(D.shape[1], idx[:n, s], val[:n, s]) for s, n in enumerate(nnz)]
    finally:
        if tmp:
            D.close()
        else:
            for key, v in saved.items():
                D.ctx.set_option(key, v)


# ------------------------------------------------------------------------------------ functors
class _Update:
    """abstract type Update; (U::Update)(x) = update!(U, x)   (src/CompressedSensing.jl:22-23)"""

    def __call__(self, x=None):
        return self.update_(x)


class _DevicePursuit(_Update):
    ALGO = None

    def __init__(self, A, b, kcap, l=1):
        self.D, self._tmp = _dict(A)
        self.A, self.b = A, np.asarray(b)
        self.l = int(l)
        M, N = self.D.shape
        self.kcap = int(kcap)
        # a context of its own that borrows the resident dictionary: like the reference's P objects, two functors on
        # one Dictionary (or a functor and a driver call) share A and nothing else
        self.ctx = self.D.ctx.clone()
        self.ctx.solver_begin(self.ALGO, b, self.kcap)
        self._x = spzeros(N)  # the x this object has been evolving

    def _sync_x(self, x):
        idx, val, res, order, stop = self.ctx.solver_state(max(self.kcap, 1))
        self._x = SparseVector(self.D.shape[1], idx, val)
        self.resnorm, self.order, self.stop = res, order, stop
        if x is None:
            return self._x.copy()
        x.nzind, x.nzval = idx.copy(), val.copy()
        return x

    def _same(self, x):
        return x is None or (x.nnz == self._x.nnz and np.array_equal(x.nzind, self._x.nzind))

    def residual_norm(self):
        return self.ctx.solver_state(max(self.kcap, 1))[2]

    def close(self):
        self.ctx.close()
        if self._tmp:
            self.D.close()


class OMP(_DevicePursuit):
    """OMP(A, b, k=size(A,1)); update!(P, x): src/matchingpursuit.jl:54-70.  The updatable QR and
    the residual live on the device, tied to the x this object returned last."""
    ALGO = _lib.ALGO_OMP

    def __init__(self, A, b, k=None):
        M = A.shape[0]
        super().__init__(A, b, M if k is None else min(int(k), M))

    def update_(self, x=None):
        if not self._same(x):
            raise ValueError("update!(P::OMP, x): x is not the support this OMP object's QR was built for")
        self.ctx.solver_step(1)
        return self._sync_x(x)


class GOMP(_DevicePursuit):
    """GOMP(A, b, l, k=size(A,1)); update!(P, x, l=P.l): src/matchingpursuit.jl:108-123."""
    ALGO = _lib.ALGO_GOMP

    def __init__(self, A, b, l, k=None):
        M = A.shape[0]
        super().__init__(A, b, M if k is None else min(int(k), M), l)

    def update_(self, x=None, l=None):
        if not self._same(x):
            raise ValueError("update!(P::GOMP, x): x is not the support this GOMP object's QR was built for")
        self.ctx.solver_step(self.l if l is None else int(l))
        return self._sync_x(x)


class FR(_DevicePursuit):
    """FR(A, b) (= OLS = OOMP = ORMP = StepwiseRegression, src/forward.jl:14-19); update!(P, x): :88-95.
    `delta2` is P.δ² of the last step (:11)."""
    ALGO = _lib.ALGO_FR

    def __init__(self, A, b, k=None):
        M = A.shape[0]
        if np.shape(b)[0] != M:
            raise ValueError(f"DimensionMismatch: size(A, 1) = {M} != {np.shape(b)[0]} = length(b)")
        super().__init__(A, b, M if k is None else min(int(k), M))

    def update_(self, x=None):
        if not self._same(x):
            raise ValueError("update!(P::FR, x): x is not the support this FR object's QR was built for")
        self.ctx.solver_step(1)
        return self._sync_x(x)

    @property
    def delta2(self):
        return self.ctx.fr_scores()


OLS = OOMP = ORMP = StepwiseRegression = FR


class MP(_DevicePursuit):
    """MP(A, b); update!(P, x): src/matchingpursuit.jl:19-31.  Any x may be passed (the reference
    recomputes the residual from x every step): a foreign x restarts the device residual from it."""
    ALGO = _lib.ALGO_MP

    def __init__(self, A, b, steps=4096):
        """steps: how many update! calls this object can record (MP keeps no factorisation, so this is only the
        length of its (atom, coefficient) log on the device)."""
        super().__init__(A, b, steps)

    def update_(self, x=None):
        if x is not None and not (self._same(x) and np.array_equal(x.nzval, self._x.nzval)):
            self.ctx.solver_begin(self.ALGO, self.b, self.kcap, x.nzind, x.nzval)
            self._base = x.copy()
        self.ctx.solver_step(1)
        idx, val, res, order, stop = self.ctx.solver_state(max(self.kcap, 1))
        base = getattr(self, "_base", None)
        out = base.copy() if base is not None else spzeros(self.D.shape[1])
        for i, v in zip(idx, val):  # steps since the (re)start, merged per atom by the library
            out[i] = out[i] + v
        self._x = out
        if x is None:
            return out.copy()
        x.nzind, x.nzval = out.nzind.copy(), out.nzval.copy()
        return x


class SBL(_Update):
    """SBL(A, b, σ²) = SparseBayesianLearning (src/sbl.jl:4-19) for a scalar noise variance; update!(S, x): :26-35, one csmp_sbl update.
    The prior variances stay on the device between the calls: `gamma` is a torch CUDA Float64 tensor, ones at the start (Γ = I).  n calls
    give the bits of sbl(A, b, σ², maxiter=n)."""

    def __init__(self, A, b, sigma2):
        _sbl_knobs(A, b, sigma2, None, 0.0)
        import torch
        self.D, self._tmp = _dict(A)
        self.A, self.b, self.sigma2 = A, np.asarray(b), float(sigma2)
        N = self.D.shape[1]
        self.ctx = self.D.ctx.clone()  # a context of its own that borrows the resident dictionary, as the pursuit functors
        self._bd = torch.from_numpy(self.ctx._b(b)).cuda()
        self.gamma = torch.ones(N, dtype=torch.float64, device="cuda")
        self._xd = torch.zeros(N, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()  # (the library works on a stream of its own)
        self.iterations = 0

    def update_(self, x=None):
        self.ctx.sbl_device(self._bd, self.sigma2, self._xd, self.gamma, self.gamma, maxiter=1, min_change=0.0)
        self.iterations += 1
        out = self._xd.cpu().numpy()
        if x is None:
            return out
        x[:] = out
        return x

    def close(self):
        self.ctx.close()
        if self._tmp:
            self.D.close()


SparseBayesianLearning = SBL


class FSBL(_Update):
    """FSBL(A, b, σ²) = FastSparseBayesianLearning (src/sbl.jl:60-87) for a scalar noise variance; update!(P): :165-176, one pass of
    csmp_fsbl (maxiter = 1) warm-started from the kept prior precisions.  `alpha` is a torch CUDA Float64 tensor, +inf (all atoms
    inactive) at the start; `x` is the posterior mean of the current α.  C⁻¹, S and Q are not kept between the calls: every call REPLAYS
    the active set -- one rank-one step per active atom -- before its pass, so a call costs (active atoms + 1) steps.  t calls give the
    history of fsbl(A, b, σ², maxiter=t)."""

    def __init__(self, A, b, sigma2):
        _fsbl_knobs("FSBL", A, b, sigma2, {}, 0.0, None)
        import torch
        self.D, self._tmp = _dict(A)
        self.A, self.b, self.sigma2 = A, np.asarray(b), float(sigma2)
        N = self.D.shape[1]
        self.ctx = self.D.ctx.clone()  # a context of its own that borrows the resident dictionary, as the pursuit functors
        self._bd = torch.from_numpy(self.ctx._b(b)).cuda()
        self.alpha = torch.full((N,), float("inf"), dtype=torch.float64, device="cuda")
        self._xd = torch.zeros(N, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()  # (the library works on a stream of its own)
        self.iterations = 0
        self.history = []

    def update_(self, x=None):
        info = self.ctx.fsbl_device(self._bd, self.sigma2, self._xd, self.alpha, self.alpha, maxiter=1, min_increase=0.0, history_cap=1)
        self.iterations += 1
        self.history += info["history"]
        out = self._xd.cpu().numpy()
        if x is None:
            return out
        x[:] = out
        return x

    @property
    def x(self):
        return self._xd.cpu().numpy()

    def close(self):
        self.ctx.close()
        if self._tmp:
            self.D.close()


FastSparseBayesianLearning = FSBL


class _TwoStage(_Update):
    """SP and OMPR: functors whose x the reference's caller owns and passes back in (update!(P, x)).  The device solver holds the x
    it produced last; an x that is not that one -- other atoms or other values -- restarts the solver from it where the reference
    allows that (SP: the acquisition starts from residual!(P, x) whatever x is, src/twostage.jl:68)."""
    ALGO = None

    def __init__(self, A, b, k):
        self.D, self._tmp = _dict(A)
        self.A, self.b, self.k = A, np.asarray(b), int(k)
        self.ctx = self.D.ctx.clone()
        self.ctx.solver_begin(self.ALGO, self.b, self.k)
        self._x = spzeros(self.D.shape[1])

    def _sync_x(self, x):
        idx, val, res, order, stop = self.ctx.solver_state(max(2 * self.k, 1))
        self._x = SparseVector(self.D.shape[1], idx, val)
        self.resnorm = res
        if x is None:
            return self._x.copy()
        x.nzind, x.nzval = idx.copy(), val.copy()
        return x

    def _is_mine(self, x):
        return x is None or (x.nnz == self._x.nnz and np.array_equal(x.nzind, self._x.nzind) and np.array_equal(x.nzval, self._x.nzval))

    def _check_nnz(self, x):
        n = self._x.nnz if x is None else x.nnz
        if n != self.k:  # the reference throws this String (src/twostage.jl:76,135)
            raise ValueError(f"nnz(x) = {n} \u2260 {self.k} = k")

    def residual_norm(self):
        return self.ctx.solver_state(max(2 * self.k, 1))[2]

    def close(self):
        self.ctx.close()
        if self._tmp:
            self.D.close()


class SP(_TwoStage):
    """SP(A, b, k) = SubspacePursuit (src/twostage.jl:42-61): sp_acquisition!(P, x, k=P.k) (:67-72) and update!(P, x) (:75-83) one
    call at a time on the device -- the phases csmp_sp strings together (sweep + top-k, least squares on the union, prune, least
    squares on the k kept)."""
    ALGO = _lib.ALGO_SP

    def __init__(self, A, b, k):
        M = A.shape[0]
        if 2 * k > M:  # error(...) at :55
            raise ValueError(f"2k = {2 * k} > {M} = length(b) is invalid for Subspace Pursuit")
        super().__init__(A, b, k)

    def _load(self, x):
        if not self._is_mine(x):  # a foreign x: the solver restarts from it (its values too: the residual is b - A x)
            self.ctx.solver_begin(self.ALGO, self.b, self.k, x.nzind, x.nzval)
            self._x = x.copy()

    def acquisition_(self, x=None, k=None):
        self._load(x)
        self.ctx.solver_acquire(self.k if k is None else int(k))
        return self._sync_x(x)

    def update_(self, x=None):
        self._check_nnz(x)
        self._load(x)
        self.ctx.solver_step(1)
        return self._sync_x(x)


SubspacePursuit = SP


class OMPR(_TwoStage):
    """OMPR(A, b, k) (src/twostage.jl:110-132): oblivious_acquisition!(P, x, k) fills the empty x (src/matchingpursuit.jl:207-216;
    how ompr starts, src/twostage.jl:190), update!(P, x) (:134-180, eta = 1) swaps one atom.  The updatable QR (with its Givens
    down-date) lives on the device, tied to the x this object returned last."""
    ALGO = _lib.ALGO_OMPR

    def acquisition_(self, x=None, k=None):
        if x is not None and x.nnz:
            raise ValueError("oblivious_acquisition!(P::OMPR, x, k): x must be empty (OMPR(A, b, k) starts from an empty factorisation)")
        if self._x.nnz:  # a fresh start of the same object
            self.ctx.solver_begin(self.ALGO, self.b, self.k)
        self.ctx.solver_acquire(self.k if k is None else int(k))
        return self._sync_x(x)

    def update_(self, x=None, eta=1.0):
        if eta != 1.0:
            raise NotImplementedError("update!(P::OMPR, x, eta): only eta = 1 (the value every driver of the reference uses) runs on the device")
        self._check_nnz(x)
        if not self._is_mine(x):
            raise ValueError("update!(P::OMPR, x): x is not the vector this OMPR object's QR was built for")
        self.ctx.solver_step(1)
        return self._sync_x(x)


def sp_acquisition(P, x=None, k=None):
    """sp_acquisition!(P::SP, x, k = P.k): src/twostage.jl:67-72"""
    return P.acquisition_(x, k)


# ------------------------------------------------------------------------------------ oblivious
def oblivious(A, b, k):
    """oblivious(A, b, k): src/oblivious.jl:3-8 -- the k atoms most correlated with b
    (partialsortperm(abs.(A'b), 1:k, rev=true)), then least squares on them.  Two device
    primitives: one sweep + top-k, one on-device QR solve.  (The reference allocates the result as
    spzeros(size(b)), i.e. of length M -- an upstream slip; here x has the dictionary's N entries.)"""
    D, tmp = _dict(A)
    try:
        _, ti, _ = D.ctx.sweep(np.asarray(b, dtype=np.float64), int(k), want_abs=False)
        coef = D.ctx.lstsq(ti, b)
        return SparseVector(D.shape[1], ti, coef)
    finally:
        if tmp:
            D.close()


def oblivious_acquisition(A, b, x=None, k=None):
    """oblivious_acquisition!(P, x, k): src/matchingpursuit.jl:207-216 -- residual of the current x,
    the k atoms best correlated with it are added (x[ind] = NaN placeholders in the reference), then
    least squares on the enlarged support.  x is updated in place and returned.
    Two call forms: (A, b, x, k) on a matrix / Dictionary, and (P, x, k) on a functor that keeps an updatable QR
    (OMPR, OMP, GOMP: csmp_solver_acquire)."""
    if isinstance(A, (_TwoStage, _DevicePursuit)):  # (P, x, k)
        P, x, k = A, b, (x if k is None else k)
        if isinstance(P, OMPR):
            return P.acquisition_(x, k)
        if not isinstance(P, (OMP, GOMP)):
            raise TypeError("oblivious_acquisition!(P, x, k): P must keep an updatable QR (OMP, GOMP, OMPR)")
        if not P._same(x):
            raise ValueError("oblivious_acquisition!(P, x, k): x is not the support this object's QR was built for")
        P.ctx.solver_acquire(int(k))
        return P._sync_x(x)
    D, tmp = _dict(A)
    try:
        b = np.asarray(b, dtype=np.float64)
        if x.nnz:
            raise NotImplementedError("oblivious_acquisition! is built for an empty x (how srr/ompr call it, "
                                      "src/twostage.jl:10,190); a non-empty x needs QR column insertion order handling")
        r = b
        _, ti, _ = D.ctx.sweep(r, int(k), want_abs=False)
        cols = np.sort(ti)
        coef = D.ctx.lstsq(cols, b)
        x.nzind, x.nzval = cols.astype(np.int64), coef
        return x
    finally:
        if tmp:
            D.close()


def random_acquisition(A, b, x, k, rng=None):
    """random_acquisition!(P, x, k): src/matchingpursuit.jl:195-204 -- k random atoms, least squares."""
    D, tmp = _dict(A)
    try:
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        cols = np.sort(rng.choice(D.shape[1], size=int(k), replace=False))
        coef = D.ctx.lstsq(cols, b)
        x.nzind, x.nzval = cols.astype(np.int64), coef
        return x
    finally:
        if tmp:
            D.close()


def update_(P, x=None, *a):
    """update!(P, x)"""
    return P.update_(x, *a)


def argmaxinner(A, r, k=None):
    """argmaxinner!(P) -> index of the largest |<a_i, r>| (first on ties);
    argmaxinner!(P, k) -> the k largest, descending, ties by ascending index (:181-193)."""
    D, tmp = _dict(A)
    try:
        _, ti, _ = D.ctx.sweep(r, 1 if k is None else int(k), want_abs=False)
        return int(ti[0]) if k is None else ti
    finally:
        if tmp:
            D.close()
