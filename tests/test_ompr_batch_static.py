"""CPU tests of csmp_ompr_batch's boundary: the header, the ctypes table, the package, the Julia wrapper, the library's exports and the
documents agree."""
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

NAME = "csmp_ompr_batch"
PROTOTYPE = """int csmp_ompr_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k,
                    const double *delta, int64_t ndelta, int64_t maxiter,
                    int64_t *idx, double *val, int64_t *nnz, int64_t *iters, int *flags);"""
NARGS = 15
GROUP_KERNELS = ("k_ompr_pick_group", "k_swap_dots_group", "k_swap_ufin_group", "k_swap_commit_res_group", "k_swap_rsum_group")


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


def test_header_declares_the_prototype():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert re.sub(r"\s+", " ", PROTOTYPE) in flat
    assert c_prototypes()[NAME] == ("i32", _params(PROTOTYPE))
    assert re.search(r"^#define CSMP_OMPR_SOLVED_ALONE 1\b", src, flags=re.M)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define CSMP_OMPR_SOLVED_ALONE 1\s*int csmp_ompr_batch\(", src, flags=re.S)
    assert m, "csmp_ompr_batch has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("bit for bit", "ndelta = 1", "ndelta = nsig", "maxiter < 0", "CSMP_OMPR_SOLVED_ALONE", "CSMP_EINVAL", "CSMP_EDIM", "CSMP_ERANGE",
                 "CSMP_ESTATE", "CSMP_ENOMEM", "nsig == 0", "CSMP_OPT_SCREENED_SWEEP", "host-streamed"):
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
    assert cs._lib.OMPR_SOLVED_ALONE == 1


def test_library_exports_the_symbol(cs):
    assert hasattr(ctypes.CDLL(cs.LIB_PATH), NAME)


def test_context_methods(cs):
    for fn in ("ompr_batch", "ompr_batch_device"):
        assert callable(getattr(cs.Context, fn)), fn
        sig = inspect.signature(getattr(cs.Context, fn))
        assert list(sig.parameters) == ["self", "B", "k", "delta", "maxiter"], fn
        assert sig.parameters["maxiter"].default is None


def test_package_exports(cs):
    assert "ompr_batch" in cs.__all__ and callable(cs.ompr_batch)
    sig = inspect.signature(cs.ompr_batch)
    assert list(sig.parameters) == ["A", "B", "k", "delta", "maxiter", "return_info"]
    for k in ("A", "B", "k", "delta"):
        assert sig.parameters[k].default is inspect.Parameter.empty
    assert sig.parameters["maxiter"].default is None and sig.parameters["return_info"].default is False
    assert inspect.signature(cs.ompr).parameters["maxiter"].default is None  # (the single call's default)


def test_python_refusals_come_before_a_device_is_touched(cs):
    A, _, b = tw.data(16, 24, 2, 0)
    B = np.asfortranarray(np.stack([b, 2.0 * b], axis=1))
    for k in (0, -1, 17, 25, 1.5, float("nan")):            # k outside 1 .. min(M, N)
        with pytest.raises(ValueError):
            cs.ompr_batch(A, B, k, 1e-6)
    for delta in (float("nan"), np.array([1e-6, np.nan]), np.ones(3), np.ones(1)[:0], np.ones((2, 1))):
        with pytest.raises(ValueError):
            cs.ompr_batch(A, B, 2, delta)
    for maxiter in (-1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            cs.ompr_batch(A, B, 2, 1e-6, maxiter=maxiter)
    with pytest.raises(ValueError):
        cs.ompr_batch(A, np.zeros((15, 2)), 2, 1e-6)        # size(B, 1) is not M
    with pytest.raises(ValueError):
        cs.ompr_batch(A, b, 2, 1e-6)                        # a vector: ompr's argument
    with pytest.raises(ValueError):
        cs.ompr_batch(A, np.zeros((16, 2, 2)), 2, 1e-6)     # more than two dimensions


def test_julia_wrapper_calls_it():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    assert re.search(r"^function ompr_batch\(A::MatOrDict, B::AbstractMatrix, k::Int, δ::Union\{Real,AbstractVector\}; maxiter::Int = size\(A, 1\)",
                     src, flags=re.M)
    assert re.search(r"^const CSMP_OMPR_SOLVED_ALONE = 1$", src, flags=re.M)
    calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:%s\s*,\s*libcsmp\s*\)" % NAME, parts[0])]
    assert len(calls) == 1
    parts = calls[0]
    assert jl_class(parts[1]) == "i32"
    types = [jl_class(t) for t in parts[2].strip()[1:-1].split(",")]
    want = _params(PROTOTYPE)
    assert len(types) == len(want) == len(parts) - 3 == NARGS
    for pos, (j, c) in enumerate(zip(types, want)):
        assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (pos, j, c)


def test_group_kernels_sit_beside_the_single_kernels():
    csrc = os.path.join(ROOT, "compressedsensing.jl_amd", "csrc")
    tinv, swap = open(os.path.join(csrc, "csmp_tinv.hpp")).read(), open(os.path.join(csrc, "csmp_swap.hpp")).read()
    assert re.search(r"__global__[^;{]*\bk_ompr_pick_group\(", tinv)
    for kern in GROUP_KERNELS[1:]:
        assert re.search(r"__global__[^;{]*\b%s\(" % kern, swap), kern
    # one body under the single kernel and the group kernel each
    for body, text in (("ompr_pick_body", tinv), ("swap_dots_body", swap), ("swap_ufin_body", swap), ("swap_commit_res_body", swap),
                       ("swap_rsum_body", swap)):
        assert len(re.findall(r"\b%s(?:<[^>]*>)?\(" % body, text)) == 3, body  # the definition and its two callers
    hip = open(os.path.join(csrc, "csmp.hip")).read()
    assert re.search(r'#include "host/twostage.hpp"\s*#include "host/ompr_batch.hpp"', hip)


def test_design_document_has_the_section():
    src = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 21\.(.*?)(?=^## \d|\Z)", src, flags=re.M | re.S)
    assert m, "DESIGN.md has no section 21"
    assert "OMP with replacement for many signals: `csmp_ompr_batch` (ompr_batch)" in m.group(0).splitlines()[0]
    for need in GROUP_KERNELS + ("CSMP_OMPR_SOLVED_ALONE", "csmp_ompr_batch", "profiles/r23_ompr_batch.json", "START", "ACQUIRE", "RUN", "FINISH",
                                 "VGPRs"):
        assert need in m.group(1), need


def test_documents_name_the_entry():
    for doc in ("README.md", "INTEGRATION.md"):
        assert "csmp_ompr_batch" in open(os.path.join(ROOT, doc)).read(), doc
    assert "r23_ompr_batch" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    tool = open(os.path.join(ROOT, "tools", "bench_ompr_batch.py")).read()
    for need in ("--baseline-root", "--mode", "--trace", "--out"):
        assert need in tool, need
