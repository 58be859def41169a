"""CPU tests of csmp_sbl's boundary -- the header, the internal header, the ctypes table, the package, the Julia wrapper, the documents and
the library's exports agree -- and of the numpy twin (tests/sbl_twin.py) that the GPU parity tests measure against: the Woodbury form
against the reference's own N × N form of the update, the recovery of the reference's test, and the conditions that make the device's
iteration count well defined."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sbl_twin as tw  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

PROTOTYPE = """int csmp_sbl(csmp_ctx *ctx, const void *b, int b_dtype, double sigma2, int64_t maxiter, double min_change,
             const double *gamma_in, double *x, double *gamma_out, int loc, int64_t *iterations, int *flags);"""
HOOKS = ("csmp_sbl_rowgram", "csmp_sbl_forms", "csmp_bench_sbl")


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ------------------------------------------------------------------------------------------ the boundary
def test_header_declares_the_prototype():
    src = _read("include", "csmp.h")
    assert re.sub(r"\s+", " ", PROTOTYPE) in re.sub(r"\s+", " ", src)
    assert c_prototypes()["csmp_sbl"] == ("i32", _params(PROTOTYPE))
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*(?:#define CSMP_SBL_[A-Z]+ \d+\s*)*int csmp_sbl\(", src, flags=re.S)
    assert m, "csmp_sbl has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("src/sbl.jl:1-51", "C = sigma2 I + A Gamma A'", "gamma_j q_j^2 / s_j + 1e-14", "zero column", "gamma_j+ = 1e-14", "min_change",
                 "128 size(A,2)", "maxiter = 1 is update!", "gamma_in", "gamma_out", "CSMP_SBL_CONVERGED", "512 MiB", "size(A,1) > size(A,2)",
                 "matrix Sigma is not served", "fsbl", "rmps", "CSMP_EINVAL", "CSMP_ERANGE", "CSMP_ESTATE", "CSMP_HOST_STREAMED", "CSMP_ENOMEM",
                 "ONE host read"):
        assert need in doc, need


def test_internal_header_declares_the_hooks():
    src = _read("include", "csmp_internal.h")
    for name in HOOKS:
        assert re.search(r"\bint %s\(csmp_ctx \*ctx," % name, src), name
    assert re.search(r"#define CSMP_TUNE_SBL_SCALAR 25\b", src)
    jl = _read("compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")  # (measurement hooks are not part of the boundary)
    assert not any(":" + name in jl for name in HOOKS)


def test_binding_table_binds_it(cs):
    C = ctypes
    res, args = cs._lib.SIGNATURES["csmp_sbl"]
    ctype = {"i32": C.c_int, "i64": C.c_int64, "f64": C.c_double}
    assert res is C.c_int
    want = _params(PROTOTYPE)
    assert len(args) == len(want) == 12
    for pos, (a, c) in enumerate(zip(args, want)):
        if c.startswith("ptr"):
            assert a is C.c_void_p or a is C.POINTER({"ptr:f64": C.c_double, "ptr:i64": C.c_int64, "ptr:i32": C.c_int}.get(c, C.c_char)), (pos, a, c)
        else:
            assert a is ctype[c], (pos, a, c)
    for name in HOOKS:
        assert name in cs._lib.INTERNAL_SIGNATURES and name not in cs._lib.SIGNATURES, name
    for fn in ("sbl", "sbl_device", "sbl_rowgram", "sbl_forms", "bench_sbl"):
        assert callable(getattr(cs.Context, fn)), fn
    assert cs._lib.TUNE["sbl_scalar"] == 25
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CSMP_SBL_[A-Z]+)\s+(\d+)", _read("include", "csmp.h"))}
    assert consts == {"CSMP_SBL_CONVERGED": cs._lib.SBL_CONVERGED}


def test_package_exports(cs):
    import inspect
    for name in ("sbl", "SBL", "SparseBayesianLearning"):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
    assert cs.SparseBayesianLearning is cs.SBL
    sig = inspect.signature(cs.sbl).parameters
    assert (sig["maxiter"].default, sig["min_change"].default, sig["return_info"].default) == (None, 1e-6, False)
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("maxiter", "min_change", "return_info"))


def test_julia_wrapper_calls_it():
    src = _read("compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")
    assert re.search(r"^function sbl\(A::MatOrDict, b::AbstractVector, σ²::Real; maxiter::Int = 128size\(A, 2\), min_change::Real = 1e-6,", src, flags=re.M)
    assert re.search(r"^const SBL = SparseBayesianLearning$", src, flags=re.M)
    assert re.search(r"^function update!\(S::SparseBayesianLearning,", src, flags=re.M)
    assert len(re.findall(r"Σ::AbstractMatrix[^\n]*a noise covariance matrix Σ is not served: scalar σ² only", src)) == 2
    calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:csmp_sbl\s*,\s*libcsmp\s*\)", parts[0])]
    assert len(calls) == 1
    parts = calls[0]
    assert jl_class(parts[1]) == "i32"
    types = [jl_class(t) for t in parts[2].strip()[1:-1].split(",")]
    want = _params(PROTOTYPE)
    assert len(types) == len(want) == len(parts) - 3
    for pos, (j, c) in enumerate(zip(types, want)):
        assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (pos, j, c)


def test_library_exports_the_symbols(cs):
    L = ctypes.CDLL(cs.LIB_PATH)
    for name in ("csmp_sbl",) + HOOKS:
        assert hasattr(L, name), name


def test_documents_say_what_is_served():
    for doc, words in (("DESIGN.md", ("## 15.", "k_sbl_forms", "k_sbl_update", "profiles/r17_sbl.json", "`fsbl`", "`rmps`")),
                       ("README.md", ("`sbl`", "`SBL`", "`fsbl`", "`rmps`", "scalar σ²")),
                       ("INTEGRATION.md", ("csmp_sbl", "`fsbl`", "`rmps`"))):
        src = _read(doc)
        for w in words:
            assert w in src, (doc, w)
    # section 7's list of what is not served no longer names SBL as a family; it names what is left of it
    design = _read("DESIGN.md")
    m = re.search(r"^## 7\..*?(?=^## 8\.)", design, flags=re.S | re.M)
    assert m and "`fsbl`" in m.group(0) and "`rmps`" in m.group(0) and "matrix Σ" in m.group(0)
    assert "dense covariance algebra" not in m.group(0)


# ------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("name", tw.DIRECT_CASES)
def test_woodbury_form_is_the_reference_update(name):
    """32x48, 100x257, 130x300 and 48x32: the same number of updates, x within 1e-12 absolute (observed: 2e-15 .. 5e-15; γ agrees to
    3e-8 relative -- the direct form cancels in 1 − diag / γ)"""
    x, i = tw.case_twin(name)
    xd, idd = tw.case_twin(name, "direct")
    dx = float(np.max(np.abs(x - xd)))
    dg = float(np.max(np.abs(i["gamma"] - idd["gamma"]) / i["gamma"]))
    print(f"{name}: updates {i['iterations']} (direct {idd['iterations']}), max|x - x_direct| = {dx:.3e}, max rel |γ - γ_direct| = {dg:.3e}")
    assert i["converged"] and idd["converged"]
    assert i["iterations"] == idd["iterations"]
    assert dx <= 1e-12


@pytest.mark.parametrize("name", sorted(tw.CASES))
def test_twin_recovers_the_planted_support(name):
    """test/sbl.jl:13-17 on every case: findall(|x| .> σ) == x0.nzind and A x ≈ b to σ"""
    A, x0, b, _ = tw.case_data(name)
    x, info = tw.case_twin(name)
    assert info["converged"] and tw.recovers(A, x, x0, b)


@pytest.mark.parametrize("name", sorted(tw.CASES))
def test_no_step_norm_lies_near_min_change(name):
    """the device's iteration count is well defined: no ‖Δγ‖ of the twin's history within 10 % of min_change"""
    _, info = tw.case_twin(name)
    h = np.array(info["history"])
    near = h[np.argmin(np.abs(np.log(h / tw.MIN_CHANGE)))]
    print(f"{name}: {info['iterations']} updates, the nearest ‖Δγ‖ to min_change = {near:.3e}")
    assert np.all((h < 0.9 * tw.MIN_CHANGE) | (h > 1.1 * tw.MIN_CHANGE)), h


def test_cases_cover_the_shapes_of_the_gpu_tests():
    shapes = {tw.CASES[n][:2] for n in tw.CASES}
    assert shapes == {(32, 48), (100, 257), (130, 300), (257, 300), (130, 1000), (48, 32)}
    for shape in shapes:
        assert {tw.CASES[n][4] for n in tw.CASES if tw.CASES[n][:2] == shape} == {np.float32, np.float64}


def test_step_form_of_the_twin():
    A, _, _, y = tw.case_data("32x48_f64")
    x3, i3 = tw.sbl(A, y, tw.SIGMA ** 2, maxiter=3)
    g = None
    for _ in range(3):
        x, i = tw.sbl(A, y, tw.SIGMA ** 2, maxiter=1, min_change=0.0, gamma=g)
        g = i["gamma"]
    assert i3["iterations"] == 3 and not i3["converged"]
    assert np.array_equal(x, x3) and np.array_equal(g, i3["gamma"])


def test_zero_column_of_the_twin():
    A, _, _, y = tw.case_data("32x48_f64")
    Z = np.array(A)
    Z[:, 5] = 0.0
    x, i = tw.sbl(Z, y, tw.SIGMA ** 2, maxiter=2)
    assert x[5] == 0.0 and i["gamma"][5] == tw.FLOOR and np.all(np.isfinite(x)) and np.all(np.isfinite(i["gamma"]))


def test_refusals_mirror_the_library(cs):
    """the twin and the package refuse the same arguments (the package before it touches a device)"""
    A, _, _, y = tw.case_data("32x48_f64")
    N = A.shape[1]
    for bad in (dict(sigma2=0.0), dict(sigma2=-1.0), dict(sigma2=float("inf")), dict(sigma2=float("nan")), dict(min_change=-1.0),
                dict(min_change=float("nan")), dict(maxiter=0)):
        kw = dict(sigma2=1e-4)
        kw.update(bad)
        s2 = kw.pop("sigma2")
        with pytest.raises(ValueError):
            tw.sbl(A, y, s2, **kw)
        with pytest.raises(ValueError):
            cs.sbl(A, y, s2, **kw)
    for s2 in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            cs.SBL(A, y, s2)
    for g in (np.zeros(N), -np.ones(N), np.r_[np.ones(N - 1), np.inf], np.r_[np.ones(N - 1), np.nan], np.ones(N - 1)):
        with pytest.raises(ValueError):
            tw.sbl(A, y, 1e-4, gamma=g)
    with pytest.raises(ValueError):
        cs.sbl(A, y[:-1], 1e-4)
    for fn in (lambda S: tw.sbl(A, y, S), lambda S: cs.sbl(A, y, S), lambda S: cs.SBL(A, y, S)):
        with pytest.raises(NotImplementedError) as e:
            fn(1e-4 * np.eye(len(y)))
        assert "a noise covariance matrix Σ is not served: scalar σ² only" in str(e.value)
