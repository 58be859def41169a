"""CPU tests of csmp_somp: the numpy twin the GPU tests compare with (tests/somp_twin.py) against the oracle and against the algorithm's
own invariants, the condition on the GPU tests' inputs (no pick is a near-tie), and the entry's boundary -- the header, the ctypes table,
the package, the Julia wrapper, the library's exports and the documents agree."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import somp_twin as tw  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

NAME = "csmp_somp"
PROTOTYPE = """int csmp_somp(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k, double eps, int p,
              int64_t *idx, double *val, int64_t ldval, int64_t *nnz, int64_t *order, double *resnorm, int64_t *passes,
              int out_loc);"""
NARGS = 17
KERNELS = ("k_somp_pick", "k_somp_project", "k_somp_solve")
RTOL = 1e-6  # the suite's tolerance against the oracle


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


# ---- the twin
@pytest.mark.parametrize("shape", list(tw.SHAPES))
def test_twin_at_one_column_is_omp(oracle, shape):
    A, B = tw.shape_data(shape)
    b = B[:, 0]
    for p in tw.PS:
        t = tw.somp(A, b[:, None], 0.0, tw.K, p)
        idx, val, order = oracle.omp(A, b, tw.K, 0.0)
        assert np.array_equal(t.order, order) and np.array_equal(t.support, idx), (shape, p)
        assert np.allclose(t.X[:, 0], val, rtol=RTOL, atol=RTOL * np.max(np.abs(val))), (shape, p)


@pytest.mark.parametrize("name", ["f32-5-p1", "f32_ragged-17-p2", "f64-9-p1", "long", "copies"])
def test_twin_invariants(name):
    c = {c.name: c for c in tw.cases()}[name]
    t = tw.reference(name)
    A, B = c.A.astype(np.float64), c.B
    assert len(t.order) == c.k == len(set(t.order.tolist())) and np.array_equal(t.support, np.sort(t.order))
    AS = A[:, t.support]
    R = B - AS @ t.X
    assert np.max(np.abs(AS.T @ R)) <= 1e-10 * np.linalg.norm(B)                 # A_S' R = 0
    X = np.linalg.lstsq(AS, B, rcond=None)[0]
    assert np.allclose(t.X, X, rtol=1e-9, atol=1e-9 * np.max(np.abs(X)))         # X is the least-squares solution on the support
    assert np.allclose(t.resnorm, np.linalg.norm(R, axis=0), rtol=1e-9)
    assert np.isclose(t.hist[-1], np.linalg.norm(R), rtol=1e-9) and np.all(np.diff(t.hist) <= 0)


def test_twin_stops_below_eps():
    shape, nsig, p = tw.EPS_CASE
    full = tw.reference(f"{shape}-{nsig}-p{p}")
    eps = 0.5 * (full.hist[5] + full.hist[6])
    assert full.hist[5] > eps > full.hist[6]
    A, B = tw.shape_data(shape)
    t = tw.somp(A, tw.columns(B, nsig), eps, tw.K, p)
    assert len(t.order) == 7 and np.array_equal(t.order, full.order[:7])


def test_no_pick_of_the_gpu_cases_is_a_near_tie():
    """a condition on the inputs: every margin (s_best - s_second) / s_best of every case is far above what a reordered Float64 sum
    can move a score by (1e-8 against ~1e-15), so the device has to make the twin's picks"""
    seen = set()
    for c in tw.cases():
        t = tw.reference(c.name)
        assert len(t.order) == c.k, c.name
        assert t.margins.min() >= 1e-8, (c.name, t.margins.min())
        seen.add(c.name)
    assert {"long", "phased", "alloc", "copies"} <= seen and len(seen) == len(tw.SHAPES) * len(tw.NSIGS) * len(tw.PS) + 4


# ---- the boundary
def test_header_declares_the_prototype():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert c_prototypes()[NAME] == ("i32", _params(PROTOTYPE))
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int csmp_somp\(", src, flags=re.S)
    assert m, "csmp_somp has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("Tropp", "p = 1 or 2", "column order", "lowest index", "CGS2", "||R||_F < eps", "One column is omp", "ldval", "order", "resnorm",
                 "passes", "group_wide", "CSMP_OPT_SCREENED_SWEEP is ignored", "host-streamed", "CSMP_EINVAL", "CSMP_ERANGE", "CSMP_ESTATE",
                 "CSMP_ENOMEM", "nsig == 0"):
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
    for fn in ("somp", "somp_device"):
        assert callable(getattr(cs.Context, fn)), fn
        sig = inspect.signature(getattr(cs.Context, fn))
        assert list(sig.parameters) == ["self", "B", "k", "eps", "p"], fn
        assert sig.parameters["p"].default == 1


def test_package_exports(cs):
    assert "somp" in cs.__all__ and callable(cs.somp)
    sig = inspect.signature(cs.somp)
    assert list(sig.parameters) == ["A", "B", "args", "max_residual", "sparsity", "p", "return_info"]
    assert sig.parameters["args"].kind is inspect.Parameter.VAR_POSITIONAL
    assert sig.parameters["max_residual"].default is None and sig.parameters["sparsity"].default is None
    assert sig.parameters["p"].default == 1 and sig.parameters["return_info"].default is False
    assert list(inspect.signature(cs.omp).parameters)[2:5] == ["args", "max_residual", "sparsity"]  # (omp's call forms)


def test_python_refusals_come_before_a_device_is_touched(cs):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((16, 24))
    B = np.asfortranarray(rng.standard_normal((16, 3)))
    for k in (0, -1, 17, 25, 1.5):                           # k outside 1 .. min(M, N)
        with pytest.raises(ValueError):
            cs.somp(A, B, 1e-3, k)
        with pytest.raises(ValueError):
            cs.somp(A, B, sparsity=k)
    for k in (0, -1, 17, 25):
        with pytest.raises(ValueError):
            cs.somp(A, B, k)
    for eps in (-1.0, -1e-300, float("nan")):                # eps < 0 or NaN
        with pytest.raises(ValueError):
            cs.somp(A, B, eps, 2)
        with pytest.raises(ValueError):
            cs.somp(A, B, max_residual=eps, sparsity=2)
    for p in (0, 3, -1, 1.0, 1.5, float("inf"), None):       # p outside {1, 2}
        with pytest.raises(ValueError):
            cs.somp(A, B, 2, p=p)
    for bad in (B[:, 0], np.zeros((15, 3)), np.zeros((16, 2, 2)), np.zeros(16)):   # B is not a matrix of M rows
        with pytest.raises(ValueError):
            cs.somp(A, bad, 2)
    with pytest.raises(TypeError):
        cs.somp(A, B, 1e-3, 2, 1)


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    assert re.search(r"^function somp\(A::MatOrDict\{T\}, B::AbstractMatrix, ε::Real, k::Int = min\(size\(A\)\.\.\.\); p::Int = 1, return_info::Bool = false\)",
                     src, flags=re.M)
    assert re.search(r"^somp\(A::MatOrDict\{T\}, B::AbstractMatrix, k::Int; kw\.\.\.\)", src, flags=re.M)
    assert re.search(r"^somp\(A::MatOrDict\{T\}, B::AbstractMatrix; max_residual = eps\(T\), sparsity = min\(size\(A\)\.\.\.\), kw\.\.\.\)", src, flags=re.M)
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
    kern = open(os.path.join(csrc, "csmp_somp.hpp")).read()
    for k in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % k, kern), k
    assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic", kern)   # no atomic operations: the same bits on every run
    host = open(os.path.join(csrc, "host", "somp.hpp")).read()
    for need in ('extern "C" int csmp_somp(', "shared_pass_launch_of<TA>", "launch_sweep(", "launch_append(ctx, 1, 0, skip, false", "CSMP_ENOMEM"):
        assert need in host, need
    hip = open(os.path.join(csrc, "csmp.hip")).read()
    assert '#include "csmp_somp.hpp"' in hip and re.search(r'#include "host/mp_batch.hpp"\s*#include "host/somp.hpp"', hip)


def test_design_document_has_the_section():
    src = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 22\.(.*?)(?=^## \d|\Z)", src, flags=re.M | re.S)
    assert m, "DESIGN.md has no section 22"
    assert "`csmp_somp` (somp)" in m.group(0).splitlines()[0]
    for need in KERNELS + ("csmp_somp", "shared_pass_launch", "k_qr1", "k_qr3", "group_wide", "bit for bit", "VGPRs"):
        assert need in m.group(1), need


def test_documents_name_the_entry():
    for doc in ("README.md", "INTEGRATION.md"):
        assert "csmp_somp" in open(os.path.join(ROOT, doc)).read(), doc
    assert "r24_somp" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    tool = open(os.path.join(ROOT, "tools", "bench_somp.py")).read()
    for need in ("--baseline-root", "--mode", "--trace", "--out"):
        assert need in tool, need
