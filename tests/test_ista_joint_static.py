"""CPU tests of csmp_ista_joint: the numpy twin the GPU tests compare with (tests/ista_joint_twin.py) against ista_twin and against the
iteration's own invariants, the condition on the GPU tests' inputs (few rows near zero, no row that a reordered sum flips), and the
entry's boundary -- the header, the ctypes table, the package, the Julia wrapper, the library's exports and the documents agree."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ista_joint_twin as tw  # noqa: E402
import ista_twin  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

NAME = "csmp_ista_joint"
PROTOTYPE = """int csmp_ista_joint(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                    const double *w, int64_t nw, const double *X0, int64_t ldX0,
                    int64_t maxiter, double stepsize, int accel,
                    double *X, int64_t ldX, int x_loc, int64_t *nrows, double *resnorm);"""
NARGS = 18
KERNELS = ("k_jista_update", "k_jista_axpy", "k_jista_resum")


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


# ---- the twin
@pytest.mark.parametrize("shape", ["32x48_f64", "256x1024_f32", "short_256x3000_f32"])
def test_twin_at_one_column_is_ista_twin(shape):
    A, _, B, alpha, _ = tw.shape_data(shape)
    b = B[:, 0]
    for lam in ista_twin.LAMBDAS:
        x = ista_twin.ista(A, b, lam, None, 64, alpha)
        X = tw.ista_joint(A, b[:, None], lam, None, 64, alpha)
        assert np.max(np.abs(X[:, 0] - x)) <= 1e-14, (shape, lam)
        assert np.array_equal(X[:, 0] != 0, x != 0), (shape, lam)
    for lam in ista_twin.FISTA_LAMBDAS:
        x = ista_twin.fista(A, b, lam, None, 64, alpha)
        X = tw.fista_joint(A, b[:, None], lam, None, 64, alpha)
        assert np.max(np.abs(X[:, 0] - x)) <= 1e-14, (shape, lam)
    w = 0.1 * np.random.default_rng(0).random(A.shape[1])
    w[::5] = 0.0
    assert np.max(np.abs(tw.ista_joint(A, b[:, None], w, None, 64, alpha)[:, 0] - ista_twin.ista(A, b, w, None, 64, alpha))) <= 1e-14


@pytest.mark.parametrize("lam", ista_twin.LAMBDAS)
def test_the_objective_of_ista_never_rises(lam):
    A, _, Ball, alpha, _ = tw.shape_data("256x1024_f32")
    B = Ball[:, :5]
    X, last = None, tw.objective(A, B, lam, np.zeros((A.shape[1], 5)))
    for _ in range(40):
        X = tw.ista_joint(A, B, lam, X, 1, alpha)
        now = tw.objective(A, B, lam, X)
        assert now <= last * (1 + 1e-13), (lam, now, last)
        last = now


def test_rows_die_and_survive_together():
    A, Xp, Ball, alpha, _ = tw.shape_data("256x1024_f32")
    X = tw.ista_joint(A, Ball[:, :9], 0.2, None, 512, alpha)
    nz = np.any(X != 0, axis=1)
    assert np.array_equal(nz, np.any(Xp != 0, axis=1))       # λ = 0.2 recovers the planted rows, and only them
    assert np.all(X[nz] != 0)                                 # a live row is scaled as a whole
    big = tw.ista_joint(A, Ball[:, :9], 1e3, None, 3, alpha)
    assert not big.any()                                      # a weight above every row norm: all rows die
    free = tw.ista_joint(A, Ball[:, :3], 0.0, None, 3, alpha)  # no weight: nothing is shrunk, the columns are ista's
    for s in range(3):
        assert np.max(np.abs(free[:, s] - ista_twin.ista(A, Ball[:, s], 0.0, None, 3, alpha))) <= 1e-14


# ---- the condition on the GPU tests' inputs
@pytest.mark.parametrize("case", tw.parity_cases(), ids=tw.case_id)
def test_the_band_condition_holds_for_every_gpu_case(case):
    """at most N/100 rows of the twin's result lie in the band ‖row‖ ≤ 1e-6 · max|X| (the parity rule's third clause, here for the twin
    alone); the result has the shape and the planted scale the rule's tolerance assumes"""
    Xt = tw.case_twin(case)
    A, B, _, _, _, _ = tw.case_args(case)
    assert Xt.shape == (A.shape[1], case.nsig) == (A.shape[1], B.shape[1])
    assert 0.1 <= np.max(np.abs(Xt)) <= 3.0
    inband = int(tw.rows_in_band(Xt, tw.band(Xt)).sum())
    print(tw.case_id(case), "rows", int(np.any(Xt != 0, axis=1).sum()), "in band", inband)
    assert inband <= Xt.shape[0] / 100
    tw.compare(Xt, Xt)


@pytest.mark.parametrize("case", [c for c in tw.parity_cases() if c.shape in ("32x48_f64", "256x1024_f32") and c.nsig in (3, 9)], ids=tw.case_id)
def test_a_reordered_sum_moves_no_row(case):
    """the twin with the summation order of Aᵀ· reversed: the device adds in yet another order, so what this moves it may move"""
    A, B, w, X0, maxiter, alpha = tw.case_args(case)
    A64 = np.asarray(A, np.float64)
    Ar = np.ascontiguousarray(A64[::-1].T)

    def reversed_At(R):
        return Ar @ R[::-1]
    X = (tw.fista_joint if case.method == "fista" else tw.ista_joint)(A, B, w, X0, maxiter, alpha, At=reversed_At)
    tw.compare(X, tw.case_twin(case))


# ---- the boundary
def test_header_declares_the_prototype():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert c_prototypes()[NAME] == ("i32", _params(PROTOTYPE))
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int %s\(" % NAME, src, flags=re.S)
    assert m, "csmp_ista_joint has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("sum_j w_j ||X[j, :]||_2", "column order", "0 exactly", "csmp_somp", "One column is csmp_ista", "ldB >= size(A,1)",
                 "ldX >= size(A,2)", "ldX0 >= size(A,2)", "X0 == X", "nrows", "resnorm", "maxiter = 0", "nsig = 0", "group_wide",
                 "CSMP_OPT_SCREENED_SWEEP is ignored", "host-streamed", "bytes a column", "CSMP_EDIM", "CSMP_EINVAL", "CSMP_ESTATE",
                 "CSMP_ENOMEM", "negative or non-finite weight", "A refused call writes nothing"):
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
    sig = inspect.signature(cs.Context.ista_joint)
    assert list(sig.parameters) == ["self", "B", "w", "X0", "maxiter", "stepsize", "accel"]
    dev = inspect.signature(cs.Context.ista_joint_device)
    assert list(dev.parameters) == ["self", "B", "w", "X", "X0", "maxiter", "stepsize", "accel"]
    one = inspect.signature(cs.Context.ista)
    for k, v in (("maxiter", 1024), ("stepsize", 1e-2), ("accel", False)):   # the defaults are csmp_ista's own
        assert one.parameters[k].default == sig.parameters[k].default == dev.parameters[k].default == v, k


def test_package_exports(cs):
    for name in ("ista_joint", "fista_joint"):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
        sig = inspect.signature(getattr(cs, name))
        assert list(sig.parameters) == ["A", "B", "lam_or_w", "X0", "maxiter", "stepsize", "return_info"]
        assert sig.parameters["X0"].default is None and sig.parameters["lam_or_w"].default is inspect.Parameter.empty
        for k, v in (("maxiter", 1024), ("stepsize", 1e-2), ("return_info", False)):
            assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == v, k
        for k in ("A", "B", "lam_or_w", "X0"):
            assert sig.parameters[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_python_refusals_come_before_a_device_is_touched(cs):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((16, 24))
    B = np.asfortranarray(rng.standard_normal((16, 3)))
    for fn in (cs.ista_joint, cs.fista_joint):
        for bad in (dict(maxiter=-1), dict(maxiter=float("nan")), dict(stepsize=0.0), dict(stepsize=-1e-2), dict(stepsize=float("inf")),
                    dict(stepsize=float("nan"))):
            with pytest.raises(ValueError):
                fn(A, B, 0.1, **bad)
        for w in (np.ones(5), np.ones(3), -np.ones(24), np.full(24, np.inf), -0.1, float("nan"), np.ones((24, 3)), np.ones((24, 1))):
            with pytest.raises(ValueError):
                fn(A, B, w)                                # (one weight per ROW: a weight per signal is not a form of this objective)
        for bad in (B[:, 0], np.zeros((15, 3)), np.zeros((16, 2, 2))):
            with pytest.raises(ValueError):
                fn(A, bad, 0.1)
        for X0 in (np.zeros((24, 2)), np.zeros((23, 3)), np.zeros(24), [cs.spzeros(24)], [cs.spzeros(24), cs.spzeros(24), cs.spzeros(23)]):
            with pytest.raises(ValueError):
                fn(A, B, 0.1, X0)


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    for name in ("ista_joint", "fista_joint"):
        assert re.search(r"^%s\(A::MatOrDict, B::AbstractMatrix, w::Union\{Real,AbstractVector\}, X0::Union\{Nothing,AbstractMatrix\} = nothing; "
                         r"maxiter::Int = 1024,\s+stepsize::Real = 1e-2, return_info::Bool = false\)" % name, src, flags=re.M), name
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
    kern = open(os.path.join(csrc, "csmp_ista_joint.hpp")).read()
    for k in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % k, kern), k
    assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic", kern)   # no atomic operations: the same bits on every run
    for need in ("ista_seg_scan(", "ista_parts(", "ista_resum_body(", "__builtin_nontemporal_load"):
        assert need in kern, need
    host = open(os.path.join(csrc, "host", "ista_joint.hpp")).read()
    for need in ('extern "C" int csmp_ista_joint(', "passes<TA>", "ista_solve(", "CSMP_ENOMEM", "CSMP_ESTATE", "bytes a column", "CHUNK AFTER CHUNK"):
        assert need in host, need
    hip = open(os.path.join(csrc, "csmp.hip")).read()
    assert re.search(r'#include "csmp_somp.hpp"\s*#include "csmp_ista_joint.hpp"', hip)
    assert re.search(r'#include "host/ista_batch.hpp"\s*#include "host/ista_joint.hpp"', hip)
    assert hip.index('#include "host/somp.hpp"') < hip.index('#include "host/ista.hpp"') < hip.index('#include "host/ista_joint.hpp"')


def test_design_document_has_the_section():
    src = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 23\.(.*?)(?=^## \d|\Z)", src, flags=re.M | re.S)
    assert m, "DESIGN.md has no section 23"
    assert "`csmp_ista_joint`" in m.group(0).splitlines()[0]
    for need in KERNELS + ("csmp_ista_joint", "shared_pass_launch", "ista_parts", "group_wide", "bit for bit", "VGPRs", "scratch",
                           "profiles/r25_ista_joint.json"):
        assert need in m.group(1), need


def test_documents_name_the_entry():
    for doc in ("README.md", "INTEGRATION.md"):
        assert "csmp_ista_joint" in open(os.path.join(ROOT, doc)).read(), doc
    assert "r25_ista_joint" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    tool = open(os.path.join(ROOT, "tools", "bench_ista_joint.py")).read()
    for need in ("--baseline-root", "--mode", "--trace", "--out"):
        assert need in tool, need
