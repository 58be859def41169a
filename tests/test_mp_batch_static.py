"""CPU tests of csmp_mp_batch's way through the layers: the header declares it, the binding table and the Julia wrapper bind it with
the header's argument types, the Python package exports mp_batch, and the built libcsmp.so exports the symbol."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototype():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+csmp_mp_batch\s*\(([^)]*)\)\s*;", src)
    assert m, "include/csmp.h does not declare csmp_mp_batch"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_header_declares_mp_batch():
    assert _prototype() == ["csmp_ctx *ctx", "const void *B", "int b_dtype", "int64_t ldB", "int64_t nsig", "int b_loc", "int64_t k",
                            "int64_t *idx", "double *val", "int64_t *nnz", "int out_loc"]
    doc = open(os.path.join(ROOT, "include", "csmp.h")).read()
    at = doc.index("int csmp_mp_batch")
    comment = doc[doc.rindex("/*", 0, at):at]
    for word in ("Warm starts", "csmp_mp", "CSMP_OPT_SCREENED_SWEEP", "nsig == 0"):  # what the header has to say about it
        assert word in comment, word


def test_binding_table_binds_mp_batch(cs):
    L = cs._lib
    res, args = L.SIGNATURES["csmp_mp_batch"]
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert res is ci and args == [vp, vp, ci, i64, i64, ci, i64, vp, vp, vp, ci]
    assert len(args) == len(_prototype())
    assert callable(L.Context.mp_batch) and callable(L.Context.mp_batch_device)


def test_package_exports_mp_batch(cs):
    assert "mp_batch" in cs.__all__ and callable(cs.mp_batch)


def test_julia_wrapper_binds_mp_batch():
    jl = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    assert re.search(r"^function mp_batch\(", jl, flags=re.M)
    m = re.search(r"ccall\(\(:csmp_mp_batch, libcsmp\), Cint,\s*\(([^)]*)\)", jl)
    assert m, "no literal ccall of csmp_mp_batch"
    types = [t.strip() for t in m.group(1).split(",")]
    assert types == ["Ptr{Cvoid}", "Ptr{Cvoid}", "Cint", "Int64", "Int64", "Cint", "Int64", "Ptr{Int64}", "Ptr{Cdouble}", "Ptr{Int64}", "Cint"]


def test_library_exports_mp_batch(cs):
    assert os.path.exists(cs.LIB_PATH), "build libcsmp.so first: python -c 'import __graft_entry__ as g; g.build()'"
    assert hasattr(ctypes.CDLL(cs.LIB_PATH), "csmp_mp_batch")
