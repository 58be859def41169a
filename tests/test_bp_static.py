"""CPU tests of csmp_bp's boundary -- the header, the ctypes table, the package, the Julia wrapper and the library's export agree --
and of the numpy twin (tests/bp_twin.py) that the GPU parity tests measure against: the twin against the linear programme."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as tw  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

PROTOTYPES = {
    "csmp_bp": """int csmp_bp(csmp_ctx *ctx, const void *b, int b_dtype, const double *w, int64_t nw,
            double rho, int64_t maxiter, double tol, int64_t check_every,
            double *x, int x_loc, int64_t *iterations, double *resnorm, int *flags);""",
    "csmp_bp_reweighted": """int csmp_bp_reweighted(csmp_ctx *ctx, const void *b, int b_dtype, int scheme, double eps, int64_t ard_iter,
                       int64_t outer_maxiter, double min_decrease, double rho, int64_t maxiter, double tol, int64_t check_every,
                       double *x, int x_loc, double *w_out, int64_t *outer_done, double *resnorm);""",
}
NARGS = {"csmp_bp": 14, "csmp_bp_reweighted": 17}


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_the_prototype(name):
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPES[name]) in flat
    assert c_prototypes()[name] == ("i32", _params(PROTOTYPES[name]))
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*(?:#define CSMP_BP_[A-Z]+ \d+\s*)*int %s\(" % name, src, flags=re.S)
    assert m, f"{name} has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    needs = {"csmp_bp": ("A x = b", "shrink", "nw = 1", "nw = size(A,2)", "CSMP_EDIM", "check_every", "CSMP_BP_CONVERGED", "CSMP_BP_FACTORED",
                         "128 MiB + 512 MiB", "not positive definite to working precision", "CSMP_ERANGE", "CSMP_HOST_STREAMED", "CSMP_ESTATE",
                         "CSMP_ENOMEM", "resnorm", "src/basispursuit.jl"),
             "csmp_bp_reweighted": ("basispursuit_reweighting", "WARM-STARTED", "min_decrease", "CSMP_ARD_KMAX", "CSMP_ERANGE")}[name]
    for need in needs:
        assert need in doc, need


def test_internal_header_declares_the_hook():
    src = open(os.path.join(ROOT, "include", "csmp_internal.h")).read()
    assert "int csmp_bp_rowgram(csmp_ctx *ctx, double *G_out, int loc);" in src
    assert "csmp_bp_rowgram" not in open(os.path.join(ROOT, "include", "csmp.h")).read()


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
    assert cs._lib.INTERNAL_SIGNATURES["csmp_bp_rowgram"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    for fn in ("bp", "bp_device", "bp_reweighted", "bp_reweighted_device", "bp_rowgram"):
        assert callable(getattr(cs.Context, fn)), fn
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CSMP_BP_[A-Z]+)\s+(\d+)", src)}
    assert consts == {"CSMP_BP_CONVERGED": cs._lib.BP_CONVERGED, "CSMP_BP_FACTORED": cs._lib.BP_FACTORED}


def test_package_exports(cs):
    for name in ("bp", "basispursuit", "bp_candes", "bp_ard"):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
    assert cs.basispursuit is cs.bp
    A, _, b = tw.data(16, 24, 2, 0)
    for bad in (dict(rho=0.0), dict(rho=float("inf")), dict(tol=0.0), dict(tol=float("nan")), dict(check_every=0), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            cs.bp(A, b, **bad)
    for w in (np.ones(5), -np.ones(24), np.full(24, np.inf)):
        with pytest.raises(ValueError):
            cs.bp(A, b, w)
    with pytest.raises(ValueError):
        cs.bp(np.asfortranarray(A.T), np.zeros(24))  # more rows than columns
    with pytest.raises(ValueError):
        cs.bp_candes(A, b, 0.0)
    with pytest.raises(ValueError):
        cs.bp_ard(A, b, iter=0)
    with pytest.raises(ValueError):
        cs.bp_candes(A, b, maxiter=0)


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    assert re.search(r"^bp\(A::MatOrDict, b::AbstractVector;", src, flags=re.M)
    assert re.search(r"^bp\(A::MatOrDict, b::AbstractVector, w::AbstractVector;", src, flags=re.M)
    assert re.search(r"^const basispursuit = bp$", src, flags=re.M)
    for fn in ("bp_candes", "bp_ard"):
        assert re.search(r"^%s\(A::MatOrDict, b::AbstractVector, ε::Real = 1e-2;" % fn, src, flags=re.M), fn
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
    for name in ("csmp_bp", "csmp_bp_reweighted", "csmp_bp_rowgram"):
        assert hasattr(L, name), name


def test_twin_generator_is_the_packages(cs):
    A, x, b = tw.data(32, 48, 3, 7, np.float32)
    A2, x2, b2 = cs.sparse_data(32, 48, 3, rng=7, dtype=np.float32)
    assert np.array_equal(A, A2) and np.array_equal(x, x2.to_dense()) and np.array_equal(b, b2)


# the twin's iteration counts at tol = 1e-9 (check_every = 32) and its distance from the LP, as found when the cases were chosen:
# recover_32x48 64 / 6e-12, weighted_100x257 160 / 5e-12, vertex_32x64 (seed 4: l1 does not recover x0) 6944 / 3.5e-9
@pytest.mark.parametrize("name", tw.STATIC_CASES)
def test_twin_agrees_with_the_linear_programme(name):
    pytest.importorskip("scipy")
    A, x0, b, w = tw.case_data(name)
    z, info = tw.case_twin(name)
    xl = tw.lp(A, b, w)
    err = float(np.max(np.abs(z - xl)))
    print(f"{name}: {info['iterations']} iterations, converged {info['converged']}, nnz {np.count_nonzero(z)}, max|z - lp| = {err:.3e}, "
          f"max|lp - x0| = {np.max(np.abs(xl - x0)):.3e}, resnorm {info['resnorm']:.3e}")
    assert info["converged"]
    assert err <= 1e-6
    M = A.shape[0]
    if name == "vertex_32x64":
        assert np.count_nonzero(z) == M and np.max(np.abs(xl - x0)) > 0.1  # a full vertex that is not x0
    else:
        assert np.array_equal(np.flatnonzero(z), np.flatnonzero(x0))
