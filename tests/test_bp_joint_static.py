"""CPU tests of csmp_bp_joint: the numpy twin the GPU tests compare with (tests/bp_joint_twin.py) against bp_twin at one column, against
the optimality conditions of  min Σ_j w_j ‖X[j, :]‖₂  s.t.  A X = B,  and against the planted rows where one column alone does not recover
them; the conditions on the GPU tests' inputs (few rows near zero, no row that a reordered sum flips); and the entry's boundary -- the
header, the ctypes table, the package, the Julia wrapper, the library's exports and the documents agree."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_joint_twin as tw  # noqa: E402
import bp_twin  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

NAME = "csmp_bp_joint"
PROTOTYPE = """int csmp_bp_joint(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                  const double *w, int64_t nw, double rho, int64_t maxiter, double tol, int64_t check_every,
                  double *X, int64_t ldX, int x_loc, int64_t *iterations, int64_t *nrows, double *resnorm, int *flags);"""
NARGS = 19
KERNELS = ("k_jbp_update", "k_jbp_pq")


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


# ---- the twin
@pytest.mark.parametrize("name", bp_twin.STATIC_CASES)
def test_twin_at_one_column_is_bp_twin(name):
    A, _, b, w = bp_twin.case_data(name)
    z, info = bp_twin.case_twin(name)
    Z, got = tw.bp_joint(A, b[:, None], w, tol=bp_twin.TWIN_TOL)
    print(name, "iterations", got["iterations"], "/ bp_twin", info["iterations"], "max|Z - z|", float(np.max(np.abs(Z[:, 0] - z))))
    assert np.max(np.abs(Z[:, 0] - z)) <= 1e-9
    assert np.array_equal(Z[:, 0] != 0, z != 0)
    assert got["converged"] and info["converged"] and got["rows"] == np.count_nonzero(z)


@pytest.mark.parametrize("shape,nsig", [("32x48_f64", 5), ("wide_130x1000_f32", 9), ("weighted_100x257_f32", 9)])
def test_the_result_satisfies_the_optimality_conditions(shape, nsig):
    """Z is feasible, and Λ with AᵀΛ = ρU (U the scaled dual of the split; at a fixed point it lies in the range of Aᵀ, so
    Λ = ρ G⁻¹ A U) is a dual certificate: ‖(AᵀΛ)[j, :]‖₂ ≤ w_j on every row, with equality and alignment to Z[j, :] on the live rows"""
    A, B, w, _ = tw.case_args(tw.Case(shape, nsig))
    A64 = np.asarray(A, np.float64)
    N = A64.shape[1]
    wv = np.ones(N) if w is None else w
    rho, st = 1.0, {}
    Z, info = tw.bp_joint(A, B, w, rho=rho, tol=tw.TWIN_TOL, state=st)
    assert info["converged"]
    feas = float(np.linalg.norm(A64 @ Z - B))
    Lam = rho * np.linalg.solve(A64 @ A64.T, A64 @ st["U"])
    D = A64.T @ Lam
    dn = np.linalg.norm(D, axis=1)
    live = np.any(Z != 0, axis=1)
    cosine = np.sum(D[live] * Z[live], axis=1) / (dn[live] * np.linalg.norm(Z[live], axis=1))
    print(shape, nsig, "‖AZ − B‖_F", feas, "max ‖(AᵀΛ)_j‖ / w_j", float(np.max(dn / wv)), "live rows", int(live.sum()),
          "min ‖·‖ / w on live", float(np.min(dn[live] / wv[live])), "min cosine", float(np.min(cosine)))
    assert feas <= 1e-8
    assert np.all(dn <= wv * (1 + 1e-6))
    assert np.all(dn[live] >= wv[live] * (1 - 1e-6))
    assert np.all(cosine >= 1 - 1e-6)


def test_joint_recovery_where_one_column_fails():
    A, X, Ball, _, _ = tw.shape_data("vertex_32x64_f64")
    planted = np.any(X != 0, axis=1)
    assert planted.sum() == 12
    Z1, info = tw.bp_joint(A, Ball[:, :1], tol=tw.TWIN_TOL)
    print("one column:", info["iterations"], "iterations,", info["rows"], "non-zeros,", float(np.linalg.norm(Z1[:, 0] - X[:, 0])), "from the planted")
    assert info["converged"] and info["rows"] == 32 and not np.array_equal(Z1[:, 0] != 0, planted)
    for nsig in (2, 3, 8, 17):
        Z, info = tw.bp_joint(A, Ball[:, :nsig], tol=tw.TWIN_TOL)
        err = float(np.max(np.abs(Z - X[:, :nsig])))
        print(nsig, "columns:", info["iterations"], "iterations,", info["rows"], "rows, max|Z − X| =", err)
        assert info["converged"] and np.array_equal(np.any(Z != 0, axis=1), planted) and err <= 1e-8


# ---- the conditions on the GPU tests' inputs
@pytest.mark.parametrize("case", tw.parity_cases(), ids=tw.case_id)
def test_the_case_conditions_hold_for_every_gpu_case(case):
    """at most N/100 rows of the twin's result lie in the band ‖row‖ ≤ 1e-6 · max|Z| (the parity rule's third clause, here for the twin
    alone); the result has the planted scale the rule's tolerance assumes; and the twin with the summation order of Aᵀ· reversed -- the
    device adds in yet another order, so what this moves it may move -- passes the parity rule and ends at the same iteration"""
    Zt, info = tw.case_twin(case)
    A, B, w, maxiter = tw.case_args(case)
    assert Zt.shape == (A.shape[1], case.nsig) == (A.shape[1], B.shape[1])
    inband = int(tw.rows_in_band(Zt, tw.band(Zt)).sum())
    print(tw.case_id(case), "iterations", info["iterations"], "converged", info["converged"], "rows", info["rows"], "in band", inband,
          "max|Z|", float(np.max(np.abs(Zt))))
    assert 0.1 <= np.max(np.abs(Zt)) <= 3.0
    assert inband <= Zt.shape[0] / 100
    assert info["converged"] == (not case.shape.startswith("ragged")) and (info["converged"] or info["iterations"] == maxiter == 64)
    A64 = np.asarray(A, np.float64)
    Ar = np.ascontiguousarray(A64[::-1].T)
    Zr, ir = tw.bp_joint(A, B, w, maxiter=maxiter, tol=tw.TWIN_TOL, At=lambda Y: Ar @ Y[::-1])
    tw.compare(Zr, Zt)
    assert ir["iterations"] == info["iterations"] and ir["converged"] == info["converged"]


# ---- the boundary
def test_header_declares_the_prototype():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert c_prototypes()[NAME] == ("i32", _params(PROTOTYPE))
    assert len(_params(PROTOTYPE)) == NARGS
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int %s\(" % NAME, src, flags=re.S)
    assert m, "csmp_bp_joint has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("min sum_j w_j ||X[j, :]||_2", "subject to A X = B", "column order", "0 exactly", "csmp_somp", "One column is csmp_bp",
                 "ldB >= size(A,1)", "ldX >= size(A,2)", "nrows", "resnorm", "maxiter = 0", "nsig = 0", "group_wide", "rule for all columns",
                 "CSMP_OPT_SCREENED_SWEEP is ignored", "host-streamed", "bytes a column", "CSMP_EDIM", "CSMP_EINVAL", "CSMP_ESTATE", "CSMP_ERANGE",
                 "CSMP_ENOMEM", "negative or non-finite weight", "not positive definite", "A refused call writes nothing"):
        assert need in doc, need


def test_binding_table_binds_it(cs):
    C = ctypes
    res, args = cs._lib.SIGNATURES[NAME]
    ctype = {"i32": C.c_int, "i64": C.c_int64, "f64": C.c_double}
    assert res is C.c_int
    want = _params(PROTOTYPE)
    assert len(args) == len(want) == NARGS
    for pos, (a, c) in enumerate(zip(args, want)):
        if c.startswith("ptr"):
            assert a is C.c_void_p or a is C.POINTER({"ptr:f64": C.c_double, "ptr:i64": C.c_int64, "ptr:i32": C.c_int}.get(c, C.c_char)), (pos, a, c)
        else:
            assert a is ctype[c], (pos, a, c)


def test_library_exports_the_symbol(cs):
    assert hasattr(ctypes.CDLL(cs.LIB_PATH), NAME)


def test_context_methods(cs):
    sig = inspect.signature(cs.Context.bp_joint)
    assert list(sig.parameters) == ["self", "B", "w", "rho", "maxiter", "tol", "check_every"]
    dev = inspect.signature(cs.Context.bp_joint_device)
    assert list(dev.parameters) == ["self", "B", "w", "X", "rho", "maxiter", "tol", "check_every"]
    one = inspect.signature(cs.Context.bp)
    for k in ("rho", "maxiter", "tol", "check_every"):   # the defaults are csmp_bp's own
        assert one.parameters[k].default == sig.parameters[k].default == dev.parameters[k].default, k


def test_package_exports(cs):
    assert "bp_joint" in cs.__all__ and callable(cs.bp_joint)
    sig = inspect.signature(cs.bp_joint)
    assert list(sig.parameters) == ["A", "B", "w", "rho", "maxiter", "tol", "check_every", "return_info"]
    assert sig.parameters["w"].default is None
    for k, v in (("rho", 1.0), ("maxiter", 16384), ("tol", 1e-8), ("check_every", 32), ("return_info", False)):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == v, k
    for k in ("A", "B", "w"):
        assert sig.parameters[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_python_refusals_come_before_a_device_is_touched(cs):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((16, 24))
    B = np.asfortranarray(rng.standard_normal((16, 3)))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(maxiter=-1), dict(maxiter=nan), dict(rho=0.0), dict(rho=-1.0), dict(rho=inf), dict(rho=nan), dict(tol=0.0), dict(tol=-1e-8),
                dict(tol=inf), dict(tol=nan), dict(check_every=0), dict(check_every=-3), dict(check_every=1.5)):
        with pytest.raises(ValueError):
            cs.bp_joint(A, B, **bad)
    for w in (np.ones(5), np.ones(3), -np.ones(24), np.full(24, inf), -0.1, nan, np.ones((24, 3)), np.ones((24, 1))):
        with pytest.raises(ValueError):
            cs.bp_joint(A, B, w)                               # (one weight per ROW: a weight per signal is not a form of this problem)
    for bad in (B[:, 0], np.zeros((15, 3)), np.zeros((16, 2, 2))):
        with pytest.raises(ValueError):
            cs.bp_joint(A, bad)
    with pytest.raises(ValueError):
        cs.bp_joint(rng.standard_normal((24, 16)), np.zeros((24, 3)))    # size(A, 1) > size(A, 2): A Aᵀ is singular


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    assert re.search(r"^bp_joint\(A::MatOrDict, B::AbstractMatrix; rho::Real = 1\.0, maxiter::Int = 16384, tol::Real = 1e-8, check_every::Int = 32, "
                     r"return_info::Bool = false\)", src, flags=re.M)
    assert re.search(r"^bp_joint\(A::MatOrDict, B::AbstractMatrix, w::Union\{Real,AbstractVector\}; rho::Real = 1\.0, maxiter::Int = 16384, "
                     r"tol::Real = 1e-8,\s+check_every::Int = 32, return_info::Bool = false\)", src, flags=re.M)
    calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:%s\s*,\s*libcsmp\s*\)" % NAME, parts[0])]
    assert len(calls) == 1
    parts = calls[0]
    assert jl_class(parts[1]) == "i32"
    types = [jl_class(t) for t in parts[2].strip()[1:-1].split(",")]
    want = _params(PROTOTYPE)
    assert len(types) == len(want) == len(parts) - 3 == NARGS
    for pos, (j, c) in enumerate(zip(types, want)):
        assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (pos, j, c)


def test_kernels_and_driver_sit_where_the_library_includes_them():
    csrc = os.path.join(ROOT, "compressedsensing.jl_amd", "csrc")
    kern = open(os.path.join(csrc, "csmp_bp_joint.hpp")).read()
    for k in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % k, kern), k
    assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic", kern)   # no atomic operations: the same bits on every run
    for need in ("bp_pq_body(", "block_sum256(", "kIstaMaxSegs + seg", "n2 = fma(t, t, n2)", "nj > tj"):
        assert need in kern, need
    host = open(os.path.join(csrc, "host", "bp_joint.hpp")).read()
    for need in ('extern "C" int csmp_bp_joint(', "passes<TA>", "residual<TA>", "bp_gemm_launch(", "k_bp_fold", "bp_prepare(", "solve_one(", "PinFetch",
                 "CSMP_ENOMEM", "CSMP_ERANGE", "bytes a column", "CHUNK AFTER CHUNK"):
        assert need in host, need
    hip = open(os.path.join(csrc, "csmp.hip")).read()
    assert re.search(r'#include "csmp_ista_joint.hpp"\s*#include "csmp_bp_joint.hpp"', hip)
    assert re.search(r'#include "host/ista_joint.hpp"\s*#include "host/bp_joint.hpp"', hip)
    assert hip.index('#include "host/bp_batch.hpp"') < hip.index('#include "host/ista_joint.hpp"') < hip.index('#include "host/bp_joint.hpp"')


def test_design_document_has_the_section():
    src = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 24\.(.*?)(?=^## \d|\Z)", src, flags=re.M | re.S)
    assert m, "DESIGN.md has no section 24"
    assert "`csmp_bp_joint`" in m.group(0).splitlines()[0]
    for need in KERNELS + ("csmp_bp_joint", "k_bp_gemm", "k_jista_axpy", "k_jista_resum", "k_bp_fold", "group_wide", "bit for bit", "VGPRs", "AGPRs",
                           "scratch", "Occupancy", "profiles/r26_bp_joint.json"):
        assert need in m.group(1), need


def test_documents_name_the_entry():
    for doc in ("README.md", "INTEGRATION.md"):
        assert "csmp_bp_joint" in open(os.path.join(ROOT, doc)).read(), doc
    tool = open(os.path.join(ROOT, "tools", "bench_bp_joint.py")).read()
    for need in ("--baseline-root", "--mode", "--trace", "--out"):
        assert need in tool, need
