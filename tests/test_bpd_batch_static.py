"""CPU tests of csmp_bpd_batch's boundary: the header, the ctypes table, the package, the Julia wrapper, the library's export and the
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

NAME = "csmp_bpd_batch"
PROTOTYPE = """int csmp_bpd_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                   const double *delta, int64_t ndelta, const double *w, int64_t nw, double rho,
                   int64_t maxiter, double tol, int64_t check_every, double *X, int64_t ldX, int x_loc,
                   int64_t *iterations, double *resnorm, int *flags);"""
NARGS = 20


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


def test_header_declares_the_prototype():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert c_prototypes()[NAME] == ("i32", _params(PROTOTYPE))
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int %s\(" % NAME, src, flags=re.S)
    assert m, "csmp_bpd_batch has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("BIT FOR BIT", "csmp_bpd(ctx, B[:, s], delta[s], ...)", "CSMP_BPD_CONVERGED", "CSMP_BPD_FACTORED", "flags[0] only",
                 "ndelta = 1", "ndelta = nsig", "ldB >= size(A,1)", "ldX >= size(A,2)", "CSMP_EDIM", "CSMP_EINVAL", "nsig = 0", "CSMP_ENOMEM",
                 "CSMP_ESTATE", "check_every", "group_max", "group_wide", "CSMP_OPT_SCREENED_SWEEP", "maxiter = 0", "non-negative and finite",
                 "size(A,1) > size(A,2) and rank-deficient dictionaries are served", "A refused call writes nothing"):
        assert need in doc, need
    # the set of flags stays the two of csmp_bpd
    assert sorted(re.findall(r"#define (CSMP_BPD_[A-Z]+) \d+", src)) == ["CSMP_BPD_CONVERGED", "CSMP_BPD_FACTORED"]


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
    for fn in ("bpd_batch", "bpd_batch_device"):
        assert callable(getattr(cs.Context, fn)), fn
    sig = inspect.signature(cs.Context.bpd_batch)
    assert list(sig.parameters) == ["self", "B", "delta", "w", "rho", "maxiter", "tol", "check_every"]
    assert sig.parameters["delta"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in ("w", "rho", "maxiter", "tol", "check_every")] == [1.0, cs._lib.BPD_RHO, 16384, 1e-8, 32]
    dev = inspect.signature(cs.Context.bpd_batch_device)
    assert list(dev.parameters) == ["self", "B", "delta", "w", "X", "rho", "maxiter", "tol", "check_every"]
    assert [dev.parameters[k].default for k in ("rho", "maxiter", "tol", "check_every")] == [cs._lib.BPD_RHO, 16384, 1e-8, 32]
    # the defaults are csmp_bpd's own
    one = inspect.signature(cs.Context.bpd)
    for k in ("w", "rho", "maxiter", "tol", "check_every"):
        assert one.parameters[k].default == sig.parameters[k].default, k


def test_package_exports(cs):
    assert "bpd_batch" in cs.__all__ and callable(cs.bpd_batch)
    sig = inspect.signature(cs.bpd_batch)
    assert list(sig.parameters) == ["A", "B", "delta", "w", "rho", "maxiter", "tol", "check_every", "return_info"]
    assert sig.parameters["w"].default is None and sig.parameters["delta"].default is inspect.Parameter.empty
    want = dict(rho=cs._lib.BPD_RHO, maxiter=16384, tol=1e-8, check_every=32, return_info=False)
    assert inspect.signature(cs.bpd).parameters["rho"].default == want["rho"] == 100.0
    for k, v in want.items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == v, k
    for k in ("A", "B", "delta", "w"):
        assert sig.parameters[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_python_refusals_come_before_a_device_is_touched(cs):
    A, _, b = tw.data(16, 24, 2, 0)
    B = np.asfortranarray(np.stack([b, 2.0 * b], axis=1))
    for bad in (dict(rho=0.0), dict(rho=float("inf")), dict(tol=0.0), dict(tol=float("nan")), dict(check_every=0), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            cs.bpd_batch(A, B, 0.1, **bad)
    for delta in (-0.1, float("nan"), float("inf"), np.ones(3), np.ones(1), np.array([0.1, -0.1]), np.array([0.1, np.inf]), np.ones((2, 1))):
        with pytest.raises(ValueError):
            cs.bpd_batch(A, B, delta)
    for w in (np.ones(5), -np.ones(24), np.full(24, np.inf), np.ones((24, 2))):
        with pytest.raises(ValueError):
            cs.bpd_batch(A, B, 0.1, w)
    with pytest.raises(ValueError):
        cs.bpd_batch(A, np.zeros((15, 2)), 0.1)                 # size(B, 1) is not M
    with pytest.raises(ValueError):
        cs.bpd_batch(A, b, 0.1)                                 # a vector: bpd's argument
    with pytest.raises(ValueError):
        cs.bpd_batch(A, np.zeros((16, 2, 2)), 0.1)              # more than two dimensions


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    assert re.search(r"^bpd_batch\(A::MatOrDict, B::AbstractMatrix, δ::Union\{Real,AbstractVector\};", src, flags=re.M)
    assert re.search(r"^bpd_batch\(A::MatOrDict, B::AbstractMatrix, δ::Union\{Real,AbstractVector\}, w::AbstractVector;", src, flags=re.M)
    assert len(re.findall(r"^bpd_batch\(.*?rho::Real = 100\.0", src, flags=re.M)) == 2
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
    m = re.search(r"^## 18\.(.*?)(?=^## \d|\Z)", src, flags=re.M | re.S)
    assert m, "DESIGN.md has no section 18"
    for need in ("k_bpd_ball_group", "k_bpd_pq_group", "csmp_bpd_batch", "profiles/r20_bpd_batch.json"):
        assert need in m.group(1), need
