"""CPU tests of csmp_ista's boundary -- the header, the ctypes table, the package, the Julia wrapper and the library's export agree --
and of the numpy twin (tests/ista_twin.py) that the GPU parity tests measure against."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ista_twin as tw  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

PROTOTYPE = """int csmp_ista(csmp_ctx *ctx, const void *b, int b_dtype, const double *w, int64_t nw,
              const int64_t *idx0, const double *val0, int64_t nnz0,
              int64_t maxiter, double stepsize, int accel,
              double *x, int x_loc, double *resnorm);"""


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


def test_header_declares_the_prototype():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert c_prototypes()["csmp_ista"] == ("i32", _params(PROTOTYPE))
    # its comment names the convention, nw, the warm start and the host-streamed refusal
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int csmp_ista\(", src, flags=re.S)
    assert m, "csmp_ista has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("||b - A x||^2 + sum_j w_j |x_j|", "shrinkage", "nw = 1", "nw = size(A,2)", "CSMP_EDIM", "warm start", "nnz0 = 0",
                 "CSMP_HOST_STREAMED", "CSMP_ESTATE", "CSMP_EINVAL", "resnorm", "src/basispursuit.jl"):
        assert need in doc, need


def test_binding_table_binds_it(cs):
    C = ctypes
    res, args = cs._lib.SIGNATURES["csmp_ista"]
    ctype = {"i32": C.c_int, "i64": C.c_int64, "f64": C.c_double}
    assert res is C.c_int
    want = _params(PROTOTYPE)
    assert len(args) == len(want) == 14
    for pos, (a, c) in enumerate(zip(args, want)):
        if c.startswith("ptr"):
            assert a is C.c_void_p or (c == "ptr:f64" and a is C.POINTER(C.c_double)), (pos, a, c)
        else:
            assert a is ctype[c], (pos, a, c)
    assert callable(cs.Context.ista) and callable(cs.Context.ista_device)


def test_package_exports(cs):
    for name in ("ista", "fista", "shrinkage"):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
    assert np.array_equal(cs.shrinkage(np.array([-2.0, -0.5, 0.0, 0.25, 3.0]), 0.5), [-1.5, 0.0, 0.0, 0.0, 2.5])
    assert cs.shrinkage(-2.0, 0.5) == -1.5
    A, _, b = tw.planted(16, 24, 2, np.float64, 0)
    with pytest.raises(ValueError):
        cs.ista(A, b, np.ones(5))
    with pytest.raises(ValueError):
        cs.ista(A, b, 0.1, maxiter=-1)
    with pytest.raises(ValueError):
        cs.fista(A, b, 0.1, stepsize=0.0)


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    for fn in ("ista", "fista"):
        assert re.search(r"^%s\(A::MatOrDict, b::AbstractVector, λ::Real" % fn, src, flags=re.M), fn
        assert re.search(r"^%s\(A::MatOrDict, b::AbstractVector, w::AbstractVector" % fn, src, flags=re.M), fn
    assert re.search(r"^shrinkage\(x::Real, α::Real\)", src, flags=re.M)
    calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:csmp_ista\s*,\s*libcsmp\s*\)", parts[0])]
    assert len(calls) == 1
    parts = calls[0]
    assert jl_class(parts[1]) == "i32"
    types = [jl_class(t) for t in parts[2].strip()[1:-1].split(",")]
    want = _params(PROTOTYPE)
    assert len(types) == len(want) == len(parts) - 3
    for pos, (j, c) in enumerate(zip(types, want)):
        assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (pos, j, c)


def test_library_exports_the_symbol(cs):
    assert hasattr(ctypes.CDLL(cs.LIB_PATH), "csmp_ista")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twin_has_the_reference_property(cs, seed):
    """test/basispursuit.jl:41-46 on seeded instances: 32 x 48, k = 3, y = perturb(b, δ/2), δ = 1e-2, λ = δ/10, stepsize = 1e-1,
    maxiter = 1024 gives ‖A x − y‖ < δ."""
    delta = 1e-2
    A, x, b = cs.sparse_data(32, 48, 3, rng=seed)
    y = cs.perturb(b, delta / 2, rng=100 + seed)
    xi = tw.ista(A, y, delta / 10, maxiter=1024, stepsize=1e-1)
    res = float(np.linalg.norm(A @ xi - y))
    print(f"seed {seed}: ‖A x − y‖ = {res:.3e}")
    assert res < delta


@pytest.mark.parametrize("case", tw.parity_cases(), ids=tw.case_id)
def test_parity_cases_have_an_empty_band(case):
    """no entry of a twin result has 0 < |x_j| ≤ atol: the band of the GPU comparison excludes nothing of the twin's own"""
    xt = tw.case_twin(case)
    atol = tw.band(xt)
    assert np.isfinite(xt).all() and atol > 0
    small = (xt != 0) & (np.abs(xt) <= atol)
    print(f"{tw.case_id(case)}: nnz = {np.count_nonzero(xt)} of {len(xt)}, max|x| = {np.abs(xt).max():.3e}, smallest non-zero = {np.abs(xt[xt != 0]).min():.3e}")
    assert not small.any(), np.flatnonzero(small)


def test_twin_fista_is_ahead_of_ista_after_200():
    """the planted case of the GPU objective test: after 200 iterations FISTA's objective is no larger than ISTA's"""
    A, _, b, alpha, _ = tw.case_data("256x1024_f32")
    fi = tw.objective(A, b, 2e-2, tw.fista(A, b, 2e-2, None, 200, alpha))
    fs = tw.objective(A, b, 2e-2, tw.ista(A, b, 2e-2, None, 200, alpha))
    print(f"objective after 200: fista {fi:.12e}  ista {fs:.12e}")
    assert fi <= fs
