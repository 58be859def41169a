"""CPU tests of csmp_fsbl_batch's and csmp_rmps_batch's boundary: the header, the ctypes table, the package, the Julia wrapper, the
library's exports and the design document agree."""
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

PROTOTYPES = {
    "csmp_fsbl_batch": """int csmp_fsbl_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                    const double *sigma2, int64_t nsigma2, int64_t maxiter, double min_increase,
                    const double *alpha_in, int64_t ld_alpha_in, double *X, int64_t ldX,
                    double *alpha_out, int64_t ld_alpha_out, int x_loc,
                    int64_t *history, int64_t history_cap, int64_t *iterations, int *flags);""",
    "csmp_rmps_batch": """int csmp_rmps_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                    const double *sigma2, int64_t nsigma2, int64_t maxiter, int64_t maxiter_acquisition,
                    int64_t maxiter_deletion, double min_increase,
                    const double *alpha_in, int64_t ld_alpha_in, double *X, int64_t ldX,
                    double *alpha_out, int64_t ld_alpha_out, int x_loc,
                    int64_t *history, int64_t history_cap, int64_t *iterations, int *flags);""",
}
NARGS = {"csmp_fsbl_batch": 21, "csmp_rmps_batch": 23}
NAMES = sorted(PROTOTYPES)


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


def test_header_declares_the_prototypes():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    for name in NAMES:
        assert re.sub(r"\s+", " ", PROTOTYPES[name]) in flat, name
        assert c_prototypes()[name] == ("i32", _params(PROTOTYPES[name])), name
    # one comment in front of the pair
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int csmp_fsbl_batch\(", src, flags=re.S)
    assert m, "csmp_fsbl_batch has no comment in front of it"
    assert re.search(r"int csmp_fsbl_batch\([^;]*;\s*int csmp_rmps_batch\(", src), "csmp_rmps_batch does not follow csmp_fsbl_batch"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("BIT FOR BIT", "csmp_fsbl(ctx, B[:, s], sigma2_s, maxiter, min_increase, alpha_in[:, s], ...)", "csmp_rmps likewise",
                 "ldB >= size(A,1)", "ldX >= size(A,2)", "ld_alpha_in >= size(A,2)", "ld_alpha_out >= size(A,2)", "nsigma2 = 1", "nsigma2 = nsig",
                 "it may be alpha_in itself", "2 history_cap s", "CSMP_EDIM", "CSMP_EINVAL", "CSMP_ESTATE", "CSMP_ERANGE", "CSMP_ENOMEM",
                 "R x size(A,1)^2 doubles", "nsig = 0", "group_max", "group_wide", "CSMP_OPT_SCREENED_SWEEP", "the message names the signal",
                 "A refused call writes nothing"):
        assert need in doc, need


@pytest.mark.parametrize("name", NAMES)
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


@pytest.mark.parametrize("solver", ["fsbl", "rmps"])
def test_context_methods_have_the_single_methods_defaults(cs, solver):
    caps = ["maxiter"] if solver == "fsbl" else ["maxiter", "maxiter_acquisition", "maxiter_deletion"]
    for fn in (solver + "_batch", solver + "_batch_device"):
        assert callable(getattr(cs.Context, fn)), fn
    one, sig = inspect.signature(getattr(cs.Context, solver)), inspect.signature(getattr(cs.Context, solver + "_batch"))
    assert list(sig.parameters) == ["self", "B", "sigma2"] + caps + ["min_increase", "alpha", "history_cap"]
    assert list(one.parameters) == ["self", "b", "sigma2"] + caps + ["min_increase", "alpha", "history_cap"]
    for k in caps + ["min_increase", "alpha", "history_cap"]:
        assert sig.parameters[k].default == one.parameters[k].default, k
    assert sig.parameters["min_increase"].default == 1e-6 and sig.parameters["history_cap"].default is None
    onedev, dev = inspect.signature(getattr(cs.Context, solver + "_device")), inspect.signature(getattr(cs.Context, solver + "_batch_device"))
    assert list(dev.parameters) == ["self", "B", "sigma2", "X", "alpha_in", "alpha_out"] + caps + ["min_increase", "history_cap"]
    assert list(onedev.parameters) == ["self", "b", "sigma2", "x", "alpha_in", "alpha_out"] + caps + ["min_increase", "history_cap"]
    for k in ["alpha_in", "alpha_out"] + caps + ["min_increase", "history_cap"]:
        assert dev.parameters[k].default == onedev.parameters[k].default, k
    assert dev.parameters["X"].default is inspect.Parameter.empty


def test_package_exports(cs):
    for name, caps in (("fsbl_batch", ["maxiter"]), ("rmps_batch", ["maxiter", "maxiter_acquisition", "maxiter_deletion"])):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
        sig = inspect.signature(getattr(cs, name))
        assert list(sig.parameters) == ["A", "B", "sigma2"] + caps + ["min_increase", "alpha", "return_info"]
        one = inspect.signature(getattr(cs, name[:-len("_batch")]))
        assert list(one.parameters) == ["A", "b", "sigma2"] + caps + ["min_increase", "alpha", "return_info"]
        for k in caps + ["min_increase", "alpha", "return_info"]:
            assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == one.parameters[k].default, k
        assert sig.parameters["min_increase"].default == 1e-6 and sig.parameters["return_info"].default is False
        for k in ("A", "B", "sigma2"):
            assert sig.parameters[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and sig.parameters[k].default is inspect.Parameter.empty


def test_python_refusals_come_before_a_device_is_touched(cs):
    A, _, b = tw.data(16, 24, 2, 0)
    B = np.asfortranarray(np.stack([b, 2.0 * b], axis=1))
    inf = np.full((24, 2), np.inf)
    for fn in (cs.fsbl_batch, cs.rmps_batch):
        caps = ["maxiter"] if fn is cs.fsbl_batch else ["maxiter", "maxiter_acquisition", "maxiter_deletion"]
        for bad in [dict(min_increase=-1e-6), dict(min_increase=float("nan"))] + [{c: v} for c in caps for v in (0, -1, 1.5, float("nan"))]:
            with pytest.raises(ValueError):
                fn(A, B, 1e-4, **bad)
        for s2 in (0.0, -1e-4, float("nan"), float("inf"), np.array([1e-4, 0.0]), np.array([1e-4, np.nan]), np.ones(3), np.ones(1)[:0]):
            with pytest.raises(ValueError):
                fn(A, B, s2)
        with pytest.raises(NotImplementedError):
            fn(A, B, np.eye(16) * 1e-4)                     # a noise covariance matrix
        with pytest.raises(ValueError):
            fn(A, np.zeros((15, 2)), 1e-4)                  # size(B, 1) is not M
        with pytest.raises(ValueError):
            fn(A, b, 1e-4)                                  # a vector: fsbl's argument
        with pytest.raises(ValueError):
            fn(A, np.zeros((16, 2, 2)), 1e-4)               # more than two dimensions
        for alpha in (np.full((24, 3), np.inf), np.full((23, 2), np.inf), np.full(24, np.inf), np.where(np.arange(48).reshape(24, 2) == 47, 0.0, inf),
                      np.where(np.arange(48).reshape(24, 2) == 5, -1.0, inf), np.where(np.arange(48).reshape(24, 2) == 5, np.nan, inf)):
            with pytest.raises(ValueError):
                fn(A, B, 1e-4, alpha=alpha)
    with pytest.raises(NotImplementedError):
        cs.rmps_batch(A, B, True)                           # the reference's Val(true)


def test_julia_wrapper_calls_them():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    assert re.search(r"^function fsbl_batch\(A::MatOrDict, B::AbstractMatrix, σ²::Union\{Real,AbstractVector\}; maxiter::Int = 2size\(A, 2\), "
                     r"min_increase::Real = 1e-6,", src, flags=re.M)
    assert re.search(r"^function rmps_batch\(A::MatOrDict, B::AbstractMatrix, σ²::Union\{Real,AbstractVector\}; maxiter::Int = size\(A, 1\),\s+"
                     r"maxiter_acquisition::Int = size\(A, 1\), maxiter_deletion::Int = size\(A, 1\), min_increase::Real = 1e-6,", src, flags=re.M)
    for name in NAMES:
        calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:%s\s*,\s*libcsmp\s*\)" % name, parts[0])]
        assert len(calls) == 1, name
        parts = calls[0]
        assert jl_class(parts[1]) == "i32"
        types = [jl_class(t) for t in parts[2].strip()[1:-1].split(",")]
        want = _params(PROTOTYPES[name])
        assert len(types) == len(want) == len(parts) - 3 == NARGS[name], name
        for pos, (j, c) in enumerate(zip(types, want)):
            assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (name, pos, j, c)


def test_library_exports_the_symbols(cs):
    lib = ctypes.CDLL(cs.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_design_document_has_the_section():
    src = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 20\.(.*?)(?=^## \d|\Z)", src, flags=re.M | re.S)
    assert m, "DESIGN.md has no section 20"
    assert "Greedy sparse Bayesian learning for many signals" in m.group(0).splitlines()[0]
    for need in ("k_fsbl_rank1_group", "k_fsbl_score_group", "k_fsbl_pick_group", "k_fsbl_col_group", "k_fsbl_gemv_group", "csmp_fsbl_batch",
                 "csmp_rmps_batch", "profiles/r22_fsbl_batch.json", "START", "REPLAY", "FINISH", "VGPRs"):
        assert need in m.group(1), need
    assert os.path.exists(os.path.join(ROOT, "profiles", "r22_fsbl_batch.json"))
