"""CPU tests of csmp_bpd's boundary -- the header, the ctypes table, the package, the Julia wrapper and the library's export agree --
and of the numpy twin (tests/bpd_twin.py) that the GPU parity tests measure against: the twin against the optimality conditions of
min Σ w|x| s.t. ‖A x − b‖ ≤ δ, a complete certificate for this convex problem when δ > 0, and against the linear programme at δ = 0."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as bt  # noqa: E402
import bpd_twin as tw  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

PROTOTYPES = {
    "csmp_bpd": """int csmp_bpd(csmp_ctx *ctx, const void *b, int b_dtype, double delta, const double *w, int64_t nw,
             double rho, int64_t maxiter, double tol, int64_t check_every,
             double *x, int x_loc, int64_t *iterations, double *resnorm, int *flags);""",
    "csmp_bpd_reweighted": """int csmp_bpd_reweighted(csmp_ctx *ctx, const void *b, int b_dtype, double delta, int scheme, double eps, int64_t ard_iter,
                        int64_t outer_maxiter, double min_decrease, double rho, int64_t maxiter, double tol, int64_t check_every,
                        double *x, int x_loc, double *w_out, int64_t *outer_done, double *resnorm);""",
}
NARGS = {"csmp_bpd": 15, "csmp_bpd_reweighted": 18}


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_the_prototype(name):
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPES[name]) in flat
    assert c_prototypes()[name] == ("i32", _params(PROTOTYPES[name]))
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*(?:#define CSMP_BPD_[A-Z]+ \d+\s*)*int %s\(" % name, src, flags=re.S)
    assert m, f"{name} has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    needs = {"csmp_bpd": ("||A x - b||_2 <= delta", "shrink", "K = I + A A'", "e - y", "nw = 1", "nw = size(A,2)", "CSMP_EDIM", "check_every",
                          "CSMP_BPD_CONVERGED", "CSMP_BPD_FACTORED", "512 MiB", "delta = 0", "delta negative or not finite", "size(A,1) > size(A,2)",
                          "CSMP_ERANGE", "CSMP_HOST_STREAMED", "CSMP_ESTATE", "CSMP_ENOMEM", "resnorm", "src/basispursuit.jl:76-100"),
             "csmp_bpd_reweighted": ("bpd_reweighting", "WARM-STARTED", "v, lam", "min_decrease = 1e-4", "eps = delta^2", "CSMP_ARD_KMAX",
                                     "CSMP_ERANGE")}[name]
    for need in needs:
        assert need in doc, need


def test_nothing_says_bpd_needs_a_cone_solver_any_more():
    for path in ("include/csmp.h", "INTEGRATION.md", "compressedsensing.jl_amd/julia/CompressedSensingAMD.jl", "DESIGN.md"):
        src = open(os.path.join(ROOT, path)).read()
        assert not re.search(r"bpd`? (needs|stays? out)", src), path


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_binding_table_binds_it(cs, name):
    C = ctypes
    res, args = cs._lib.SIGNATURES[name]
    ctype = {"i32": C.c_int, "i64": C.c_int64, "f64": C.c_double}
    assert res is C.c_int
    want = _params(PROTOTYPES[name])
    assert len(args) == len(want) == NARGS[name]
    for pos, (a, c) in enumerate(zip(args, want)):
        if c.startswith("ptr"):
            assert a is C.c_void_p or a is C.POINTER({"ptr:f64": C.c_double, "ptr:i64": C.c_int64, "ptr:i32": C.c_int}.get(c, C.c_char)), (pos, a, c)
        else:
            assert a is ctype[c], (pos, a, c)
    for fn in ("bpd", "bpd_device", "bpd_reweighted", "bpd_reweighted_device"):
        assert callable(getattr(cs.Context, fn)), fn
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CSMP_BPD_[A-Z]+)\s+(\d+)", src)}
    assert consts == {"CSMP_BPD_CONVERGED": cs._lib.BPD_CONVERGED, "CSMP_BPD_FACTORED": cs._lib.BPD_FACTORED}


def test_package_exports(cs):
    import inspect
    for name in ("bpd", "basis_pursuit_denoising", "bpd_candes", "bpd_ard"):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
    assert cs.basis_pursuit_denoising is cs.bpd
    sig = inspect.signature(cs.bpd).parameters
    assert (sig["maxiter"].default, sig["tol"].default, sig["check_every"].default, sig["w"].default) == (16384, 1e-8, 32, None)
    for fn in (cs.bpd_candes, cs.bpd_ard):
        sig = inspect.signature(fn).parameters
        assert sig["min_decrease"].default == 1e-4 and sig["eps"].default is None and sig["maxiter"].default == 8
    # the default penalty is the one with the smallest total of DESIGN.md's iteration table, in all three bindings
    rho = inspect.signature(cs.bpd).parameters["rho"].default
    assert rho == inspect.signature(cs.Context.bpd).parameters["rho"].default == inspect.signature(cs.bpd_ard).parameters["rho"].default == 100.0
    A, _, b = bt.data(16, 24, 2, 0)
    for bad in (dict(rho=0.0), dict(rho=float("inf")), dict(tol=0.0), dict(tol=float("nan")), dict(check_every=0), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            cs.bpd(A, b, 1e-2, **bad)
    for delta in (-1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            cs.bpd(A, b, delta)
        with pytest.raises(ValueError):
            cs.bpd_candes(A, b, delta)
    for w in (np.ones(5), -np.ones(24), np.full(24, np.inf)):
        with pytest.raises(ValueError):
            cs.bpd(A, b, 1e-2, w)
    with pytest.raises(ValueError):
        cs.bpd_candes(A, b, 1e-2, 0.0)
    with pytest.raises(ValueError):
        cs.bpd_candes(A, b, 0.0)  # eps = delta = 0
    with pytest.raises(ValueError):
        cs.bpd_ard(A, b, 1e-2, iter=0)
    with pytest.raises(ValueError):
        cs.bpd_candes(A, b, 1e-2, maxiter=0)


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    assert re.search(r"^bpd\(A::MatOrDict, b::AbstractVector, δ::Real;", src, flags=re.M)
    assert re.search(r"^bpd\(A::MatOrDict, b::AbstractVector, δ::Real, w::AbstractVector;", src, flags=re.M)
    assert re.search(r"^const basis_pursuit_denoising = bpd$", src, flags=re.M)
    assert re.search(r"^bpd_candes\(A::MatOrDict, b::AbstractVector, δ::Real, ε::Real = δ; maxiter::Int = 8, min_decrease::Real = 1e-4,", src, flags=re.M)
    assert re.search(r"^bpd_ard\(A::MatOrDict, b::AbstractVector, δ::Real, ε::Real = δ\^2; maxiter::Int = 8, min_decrease::Real = 1e-4,", src, flags=re.M)
    for name in sorted(PROTOTYPES):
        calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:%s\s*,\s*libcsmp\s*\)" % name, parts[0])]
        assert len(calls) == 1, name
        parts = calls[0]
        assert jl_class(parts[1]) == "i32"
        types = [jl_class(t) for t in parts[2].strip()[1:-1].split(",")]
        want = _params(PROTOTYPES[name])
        assert len(types) == len(want) == len(parts) - 3
        for pos, (j, c) in enumerate(zip(types, want)):
            assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (name, pos, j, c)


def test_library_exports_the_symbols(cs):
    L = ctypes.CDLL(cs.LIB_PATH)
    for name in ("csmp_bpd", "csmp_bpd_reweighted"):
        assert hasattr(L, name), name


# ------------------------------------------------------------------------------------------ the twin
# The twin's iterations at tol = 1e-9, check_every = 32, ρ = 100, and the three certificate figures, as found when the cases were chosen:
#   recover_32x48 192 (2.6e-13, 3.9e-12, 0.946), weighted_100x257 288 (1.9e-12, 1.4e-10, 0.993), vertex_32x64 3104 (6.7e-12, 4.2e-10, 0.929),
#   tall_48x32 128 (5.0e-14, 2.8e-13, 0.943); wide_130x1000 (GPU test only) 352 (1.3e-11, 1.3e-10, 0.99974); ragged_257x300 160
@pytest.mark.parametrize("name", tw.STATIC_CASES)
def test_twin_passes_the_optimality_certificate(name):
    A, _, b, w, delta = tw.case_data(name)
    z, info = tw.case_twin(name)
    feas, on, off = tw.certificate(A, b, delta, w, z)
    print(f"{name}: {info['iterations']} iterations, nnz {np.count_nonzero(z)}, min|z_j| = {np.min(np.abs(z[z != 0])):.3e}; | ||r|| - δ | / δ = {feas:.3e}, "
          f"on the support {on:.3e}, off it {off:.6f}")
    assert info["converged"]
    assert feas <= 1e-6
    assert on <= 1e-6
    assert off <= 1 + 1e-6


def test_twin_returns_zero_inside_the_ball():
    A, _, b, w, delta = tw.case_data("zero")
    assert delta >= np.linalg.norm(b)
    z, info = tw.case_twin("zero")
    assert info["converged"] and not np.any(z) and info["resnorm"] == np.linalg.norm(b)


def test_twin_at_delta_zero_agrees_with_the_linear_programme():
    pytest.importorskip("scipy")
    A, x0, b, w = bt.case_data("recover_32x48")
    z, info = tw.bpd(A, b, 0.0, w, rho=tw.RHO, tol=tw.TWIN_TOL)
    xl = bt.lp(A, b, w)
    err = float(np.max(np.abs(z - xl)))
    print(f"δ = 0: {info['iterations']} iterations, converged {info['converged']}, nnz {np.count_nonzero(z)}, max|z - lp| = {err:.3e}")
    assert info["converged"]
    assert err <= 1e-6
    assert np.array_equal(np.flatnonzero(z), np.flatnonzero(x0))


def test_twin_reweighted_recovers_the_planted_support():
    A, x0, b, _, delta = tw.case_data("recover_32x48")
    for scheme in ("candes", "ard"):
        z, w, done, its = tw.case_reweighted("recover_32x48", scheme, 3, 0.0)
        print(f"{scheme}: solves {done}, iterations {its}")
        assert done == 3 and np.array_equal(np.flatnonzero(z), np.flatnonzero(x0))
        assert np.linalg.norm(A.astype(np.float64) @ z - b) <= delta * (1 + 1e-6)
