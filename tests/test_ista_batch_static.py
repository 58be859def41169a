"""CPU tests of csmp_ista_batch's boundary: the header, the ctypes table, the package, the Julia wrapper, the library's export and the
design document agree."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as tw  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

NAME = "csmp_ista_batch"
PROTOTYPE = """int csmp_ista_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                    const double *w, int64_t nw, int64_t ldw, const double *X0, int64_t ldX0,
                    int64_t maxiter, double stepsize, int accel, double *X, int64_t ldX, int x_loc,
                    double *resnorm);"""
NARGS = 18


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


def test_header_declares_the_prototype():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert c_prototypes()[NAME] == ("i32", _params(PROTOTYPE))
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int %s\(" % NAME, src, flags=re.S)
    assert m, "csmp_ista_batch has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("BIT FOR BIT", "csmp_ista(ctx, B[:, s], w_s, x0_s, maxiter, stepsize, accel, ...)", "ldB >= size(A,1)", "ldX >= size(A,2)",
                 "ldX0 >= size(A,2)", "ldw = 0", "ldw >= nw", "X0 == X", "CSMP_EDIM", "CSMP_EINVAL", "CSMP_ESTATE", "CSMP_ENOMEM", "nsig = 0",
                 "maxiter = 0", "group_max", "group_wide", "CSMP_OPT_SCREENED_SWEEP", "negative or non-finite weight",
                 "A refused call writes nothing"):
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
    for fn in ("ista_batch", "ista_batch_device"):
        assert callable(getattr(cs.Context, fn)), fn
    sig = inspect.signature(cs.Context.ista_batch)
    assert list(sig.parameters) == ["self", "B", "w", "X0", "maxiter", "stepsize", "accel"]
    assert sig.parameters["w"].default is inspect.Parameter.empty and sig.parameters["X0"].default is None
    dev = inspect.signature(cs.Context.ista_batch_device)
    assert list(dev.parameters) == ["self", "B", "w", "X", "X0", "maxiter", "stepsize", "accel"]
    assert dev.parameters["X"].default is inspect.Parameter.empty and dev.parameters["X0"].default is None
    # the defaults are csmp_ista's own
    one = inspect.signature(cs.Context.ista)
    for k, v in (("maxiter", 1024), ("stepsize", 1e-2), ("accel", False)):
        assert one.parameters[k].default == sig.parameters[k].default == dev.parameters[k].default == v, k


def test_package_exports(cs):
    for name in ("ista_batch", "fista_batch"):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
        sig = inspect.signature(getattr(cs, name))
        assert list(sig.parameters) == ["A", "B", "lam_or_w", "X0", "maxiter", "stepsize"]
        assert sig.parameters["X0"].default is None and sig.parameters["lam_or_w"].default is inspect.Parameter.empty
        one = inspect.signature(getattr(cs, name[:-len("_batch")]))
        for k, v in (("maxiter", 1024), ("stepsize", 1e-2)):
            assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == one.parameters[k].default == v, k
        for k in ("A", "B", "lam_or_w", "X0"):
            assert sig.parameters[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_the_weights_forms(cs):
    f = cs._lib.ista_batch_weights
    N, nsig = 24, 3
    w, nw, ldw = f(0.5, N, nsig)
    assert (w.tolist(), nw, ldw) == ([0.5], 1, 0)
    w, nw, ldw = f(np.arange(N), N, nsig)
    assert (w.shape, nw, ldw) == ((N,), N, 0)
    w, nw, ldw = f([0.1, 0.2, 0.1], N, nsig)
    assert (w.tolist(), nw, ldw) == ([0.1, 0.2, 0.1], 1, 1)
    W = np.arange(N * nsig, dtype=np.float64).reshape(nsig, N).T      # (not Fortran-ordered as it comes)
    w, nw, ldw = f(W, N, nsig)
    assert w.flags.f_contiguous and np.array_equal(w, W) and (nw, ldw) == (N, N)
    w, nw, ldw = f(np.arange(N), N, N)                                # nsig == N: the shared N-vector
    assert (nw, ldw) == (N, 0)


def test_python_refusals_come_before_a_device_is_touched(cs):
    A, _, b = tw.data(16, 24, 2, 0)
    B = np.asfortranarray(np.stack([b, 2.0 * b], axis=1))
    for fn in (cs.ista_batch, cs.fista_batch):
        for bad in (dict(maxiter=-1), dict(maxiter=float("nan")), dict(stepsize=0.0), dict(stepsize=-1e-2), dict(stepsize=float("inf")),
                    dict(stepsize=float("nan"))):
            with pytest.raises(ValueError):
                fn(A, B, 0.1, **bad)
        for w in (np.ones(5), np.ones(3), -np.ones(24), np.full(24, np.inf), -0.1, float("nan"), np.array([0.1, -0.1]), np.array([0.1, np.nan]),
                  np.ones((24, 3)), np.ones((2, 24)), np.ones((24, 2, 1)), -np.ones((24, 2))):
            with pytest.raises(ValueError):
                fn(A, B, w)
        with pytest.raises(ValueError):
            fn(A, np.zeros((15, 2)), 0.1)                 # size(B, 1) is not M
        with pytest.raises(ValueError):
            fn(A, b, 0.1)                                 # a vector: ista's argument
        with pytest.raises(ValueError):
            fn(A, np.zeros((16, 2, 2)), 0.1)              # more than two dimensions
        for X0 in (np.zeros((24, 3)), np.zeros((23, 2)), np.zeros(24), [cs.spzeros(24)], [cs.spzeros(24), cs.spzeros(23)]):
            with pytest.raises(ValueError):
                fn(A, B, 0.1, X0)


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    for name in ("ista_batch", "fista_batch"):
        assert re.search(r"^%s\(A::MatOrDict, B::AbstractMatrix, w::Union\{Real,AbstractVecOrMat\}, X0::Union\{Nothing,AbstractMatrix\} = nothing; "
                         r"maxiter::Int = 1024,\s+stepsize::Real = 1e-2\)" % name, src, flags=re.M), name
    calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:%s\s*,\s*libcsmp\s*\)" % NAME, parts[0])]
    assert len(calls) == 1
    parts = calls[0]
    assert jl_class(parts[1]) == "i32"
    types = [jl_class(t) for t in parts[2].strip()[1:-1].split(",")]
    want = _params(PROTOTYPE)
    assert len(types) == len(want) == len(parts) - 3 == NARGS
    for pos, (j, c) in enumerate(zip(types, want)):
        assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (pos, j, c)


def test_library_exports_the_symbol(cs):
    assert hasattr(ctypes.CDLL(cs.LIB_PATH), NAME)


def test_design_document_has_the_section():
    src = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 19\.(.*?)(?=^## \d|\Z)", src, flags=re.M | re.S)
    assert m, "DESIGN.md has no section 19"
    assert "l1 solves for many signals" in m.group(0).splitlines()[0]
    for need in ("k_ista_update_group", "csmp_ista_batch", "profiles/r21_ista_batch.json"):
        assert need in m.group(1), need
