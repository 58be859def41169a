"""CPU tests of csmp_fsbl's and csmp_rmps' boundary -- the header, the internal header, the ctypes table, the package, the Julia wrapper,
the documents and the library's exports agree -- and of the numpy twin (tests/fsbl_twin.py) that the GPU parity tests measure against: the
recurrences against a from-scratch form, x = Q / α against the reference's solve, the recovery of the reference's test, and the conditions
that make the device's trajectory well defined."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsbl_twin as tw  # noqa: E402
import sbl_twin as st  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

PROTOTYPES = {
    "csmp_fsbl": """int csmp_fsbl(csmp_ctx *ctx, const void *b, int b_dtype, double sigma2, int64_t maxiter, double min_increase,
              const double *alpha_in, double *x, double *alpha_out, int loc,
              int64_t *history, int64_t history_cap, int64_t *iterations, int *flags);""",
    "csmp_rmps": """int csmp_rmps(csmp_ctx *ctx, const void *b, int b_dtype, double sigma2, int64_t maxiter, int64_t maxiter_acquisition,
              int64_t maxiter_deletion, double min_increase, const double *alpha_in, double *x, double *alpha_out, int loc,
              int64_t *history, int64_t history_cap, int64_t *iterations, int *flags);""",
}
HOOKS = ("csmp_fsbl_score", "csmp_fsbl_sqc", "csmp_bench_fsbl")
S2 = tw.SIGMA ** 2


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ------------------------------------------------------------------------------------------ the boundary
def test_header_declares_the_prototypes():
    src = _read("include", "csmp.h")
    flat = re.sub(r"\s+", " ", src)
    for name, proto in PROTOTYPES.items():
        assert re.sub(r"\s+", " ", proto) in flat, name
        assert c_prototypes()[name] == ("i32", _params(proto)), name
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*(?:#define CSMP_(?:FSBL|RMPS)_[A-Z]+ \d+\s*)*int csmp_fsbl\(", src, flags=re.S)
    assert m, "csmp_fsbl has no comment in front of it"
    doc = re.sub(r"\s+", " ", m.group(1))
    for need in ("src/sbl.jl:57-437", "alpha / (alpha - S)", "s^2 / (q^2 - s)", "C^-1 -= v v' / den", "S -= w^2 / den", "Q -= w Q_i / den",
                 "min_increase", "2 size(A,2)", "maxiter = 1 is update!", "maxiter_acquisition", "maxiter_deletion", "alpha_in", "alpha_out",
                 "history_cap", "1 add, 2 delete, 3 re-estimate", "CSMP_FSBL_CONVERGED", "CSMP_RMPS_CONVERGED", "Q_j / alpha_j", "128 MiB",
                 "matrix Sigma", "sigma2-optimising", "rmp_acquisition_value", "CSMP_EINVAL", "CSMP_ERANGE", "CSMP_ESTATE",
                 "CSMP_HOST_STREAMED", "CSMP_ENOMEM", "ONE host read"):
        assert need in doc, need
    # no new constant is named CSMP_SBL_*
    assert set(re.findall(r"#define (CSMP_SBL_[A-Z_]+)", src)) == {"CSMP_SBL_CONVERGED"}
    consts = dict(re.findall(r"#define (CSMP_(?:FSBL|RMPS)_[A-Z_]+)\s+(\d+)", src))
    assert consts == {"CSMP_FSBL_CONVERGED": "1", "CSMP_RMPS_CONVERGED": "1"}


def test_internal_header_declares_the_hooks():
    src = _read("include", "csmp_internal.h")
    pub = _read("include", "csmp.h")
    for name in HOOKS:
        assert re.search(r"\bint %s\(csmp_ctx \*ctx," % name, src), name
        assert not re.search(r"\b%s\(" % name, pub), name
    assert re.search(r"#define CSMP_TUNE_SBL_SCALAR 25\b", src)
    assert re.search(r"#define CSMP_TUNE_FSBL_SCALAR 26\b", src)
    jl = _read("compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")  # (measurement hooks are not part of the boundary)
    assert not any(":" + name in jl for name in HOOKS)


def test_binding_table_binds_them(cs):
    C = ctypes
    ctype = {"i32": C.c_int, "i64": C.c_int64, "f64": C.c_double}
    for name, proto in PROTOTYPES.items():
        res, args = cs._lib.SIGNATURES[name]
        assert res is C.c_int
        want = _params(proto)
        assert len(args) == len(want) == (14 if name == "csmp_fsbl" else 16)
        for pos, (a, c) in enumerate(zip(args, want)):
            if c.startswith("ptr"):
                assert a is C.c_void_p or a is C.POINTER({"ptr:f64": C.c_double, "ptr:i64": C.c_int64, "ptr:i32": C.c_int}.get(c, C.c_char)), (pos, a, c)
            else:
                assert a is ctype[c], (name, pos, a, c)
    for name in HOOKS:
        assert name in cs._lib.INTERNAL_SIGNATURES and name not in cs._lib.SIGNATURES, name
    for fn in ("fsbl", "rmps", "fsbl_device", "rmps_device", "fsbl_score", "fsbl_sqc", "bench_fsbl"):
        assert callable(getattr(cs.Context, fn)), fn
    assert cs._lib.TUNE["fsbl_scalar"] == 26 and cs._lib.TUNE["sbl_scalar"] == 25
    assert cs._lib.FSBL_CONVERGED == cs._lib.RMPS_CONVERGED == 1
    assert cs._lib.FSBL_MODES == {"all": tw.ALL, "add": tw.ADD, "rmp_delete": tw.RMP_DEL, "update": tw.UPD}


def test_package_exports(cs):
    import inspect
    for name in ("fsbl", "rmps", "FSBL", "FastSparseBayesianLearning"):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
    assert cs.FastSparseBayesianLearning is cs.FSBL
    sig = inspect.signature(cs.fsbl).parameters
    assert list(sig) == ["A", "b", "sigma2", "maxiter", "min_increase", "alpha", "return_info"]
    assert [sig[k].default for k in ("maxiter", "min_increase", "alpha", "return_info")] == [None, 1e-6, None, False]
    sig = inspect.signature(cs.rmps).parameters
    assert list(sig) == ["A", "b", "sigma2", "maxiter", "maxiter_acquisition", "maxiter_deletion", "min_increase", "alpha", "return_info"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, None, None, 1e-6, None, False]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for fn in (cs.fsbl, cs.rmps) for p in list(inspect.signature(fn).parameters.values())[3:])
    assert "replays the active set".lower() in re.sub(r"\s+", " ", cs.FSBL.__doc__).lower()


def test_julia_wrapper_calls_them():
    src = _read("compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")
    assert re.search(r"^function fsbl\(A::MatOrDict, b::AbstractVector, σ²::Real; maxiter::Int = 2size\(A, 2\), min_increase::Real = 1e-6,", src, flags=re.M)
    assert re.search(r"^function rmps\(A::MatOrDict, b::AbstractVector, σ²::Real; maxiter::Int = size\(A, 1\), maxiter_acquisition::Int = size\(A, 1\),",
                     src, flags=re.M)
    for fn in ("fsbl", "rmps"):  # a matrix Σ is refused, in words of their own (tests/test_sbl_static.py counts sbl's)
        assert re.search(r"^%s\(A::MatOrDict, b::AbstractVector, Σ::AbstractMatrix; kwargs\.\.\.\) = error\(" % fn, src, flags=re.M), fn
    assert re.search(r"^rmps\(A::MatOrDict, b::AbstractVector, ::Val\{true\}, args\.\.\.; kwargs\.\.\.\) = error\(", src, flags=re.M)
    assert len(re.findall(r"Σ::AbstractMatrix[^\n]*a noise covariance matrix Σ is not served: scalar σ² only", src)) == 2
    for name, proto in PROTOTYPES.items():
        calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:%s\s*,\s*libcsmp\s*\)" % name, parts[0])]
        assert len(calls) == 1, name
        parts = calls[0]
        assert jl_class(parts[1]) == "i32"
        types = [jl_class(t) for t in re.sub(r"\s+", "", parts[2])[1:-1].split(",")]
        want = _params(proto)
        assert len(types) == len(want) == len(parts) - 3, name
        for pos, (j, c) in enumerate(zip(types, want)):
            assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (name, pos, j, c)


def test_library_exports_the_symbols(cs):
    L = ctypes.CDLL(cs.LIB_PATH)
    for name in tuple(PROTOTYPES) + HOOKS:
        assert hasattr(L, name), name


def test_documents_say_what_is_served():
    for doc, words in (("DESIGN.md", ("## 16.", "k_fsbl_score", "k_fsbl_pick", "k_fsbl_col", "k_fsbl_rank1", "profiles/r18_fsbl.json", "csmp_fsbl",
                                      "csmp_rmps")),
                       ("README.md", ("`fsbl`", "`rmps`", "`FSBL`", "scalar σ²")),
                       ("INTEGRATION.md", ("csmp_fsbl", "csmp_rmps", "`fsbl`", "`rmps`")),
                       (os.path.join("profiles", "README.md"), ("r18_fsbl.json", "tools/bench_fsbl.py"))):
        src = _read(doc)
        for w in words:
            assert w in src, (doc, w)
    # the sentences that said "not served" are gone
    for doc, gone in ((("include", "csmp.h"), "are not served either"), (("compressedsensing.jl_amd", "api.py"), "fsbl and rmps are not served"),
                      (("compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl"), "nor are fsbl and rmps"),
                      (("README.md",), "(`NotImplementedError`), `fsbl` and `rmps`"), (("INTEGRATION.md",), "`fsbl` and `rmps` (`:57-470`)"),
                      (("DESIGN.md",), "stay out: they were tried once"), (("DESIGN.md",), "`fsbl`, `rmps` and a matrix Σ are not served")):
        assert gone not in re.sub(r"\s+", " ", _read(*doc)), doc
    m = re.search(r"^## 7\..*?(?=^## 8\.)", _read("DESIGN.md"), flags=re.S | re.M)
    assert m and "σ²-optimising" in m.group(0)


# ------------------------------------------------------------------------------------------ the twin
def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("name,solver", tw.RUNS)
def test_recurrences_against_the_from_scratch_form(name, solver):
    """after every step S, Q and C⁻¹ of the recurrences agree with a dense inverse of σ² I + A_a Γ_a A_aᵀ to 1e-8 of the largest entry"""
    A, _, _, y = tw.case_data(name)
    dS, dQ, dC = tw.drift(np.asarray(A, np.float64), y, S2, solver)
    print(f"{name} {solver}: drift of S {dS:.3e}, Q {dQ:.3e}, C⁻¹ {dC:.3e}")
    assert max(dS, dQ, dC) <= 1e-8


@pytest.mark.parametrize("name,solver", tw.RUNS)
def test_x_is_the_reference_solve(name, solver):
    A, _, _, y = tw.case_data(name)
    x, info = tw.case_twin(name, solver)
    xs = tw.solve_x(np.asarray(A, np.float64), y, S2, info["alpha"])
    print(f"{name} {solver}: max|Q/α − solve| / max|x| = {_rel(x, xs):.3e}")
    assert np.array_equal(x != 0, np.isfinite(info["alpha"]))
    assert _rel(x, xs) <= 1e-9


@pytest.mark.parametrize("solver", ["fsbl", "rmps"])
@pytest.mark.parametrize("name", sorted(st.CASES))
def test_twin_recovers_the_planted_support(name, solver):
    """test/sbl.jl:20-27 on the twelve cases of sbl_twin: the entries above σ are the planted support and A x ≈ b to σ"""
    A, x0, b, _ = tw.case_data(name)
    x, info = tw.case_twin(name, solver)
    assert info["converged"] and st.recovers(A, x, x0, b)
    assert not any(a == tw.ACT_DEL for a, _ in info["history"])
    assert tw.case_twin(name, "fsbl")[1]["history"] == tw.case_twin(name, "rmps")[1]["history"]


@pytest.mark.parametrize("name,solver", tw.RUNS)
def test_the_trajectory_is_well_defined(name, solver):
    """what lets the device -- whose S and Q differ from the twin's in the last bits -- take the same decisions (fsbl_twin.conditions):
    every pick that counts is ahead of the runner-up by 1e-6 relative, no deletion value within 1e-3 of 1, no value compared with
    min_increase within a factor 2 of it, and the relevance test s < q² of every atom acted on is decided by more than 1e-6 q²"""
    _, info = tw.case_twin(name, solver)
    gap, near1, nearmin, rel = tw.conditions(info)
    print(f"{name} {solver}: smallest gap to the runner-up {gap:.3e}, deletion value nearest to 1 off by {near1:.3e}, "
          f"value nearest to min_increase off by a factor {nearmin:.3f}, |s − q²| / q² ≥ {rel:.3e}")
    assert info["converged"]
    assert gap >= 1e-6 and near1 >= 1e-3 and nearmin >= 2.0 and rel >= 1e-6


def test_cases_cover_deletions_and_both_drivers():
    dels = {n for n, s in tw.RUNS if any(a == tw.ACT_DEL for a, _ in tw.case_twin(n, s)[1]["history"])}
    assert len({n.rsplit("_", 1)[0] for n in dels}) >= 3, dels
    differ = [n for n in tw.CASES if tw.case_twin(n, "fsbl")[1]["history"] != tw.case_twin(n, "rmps")[1]["history"]]
    assert differ
    assert {tw.CASES[n][:2] for n in tw.CASES} == {(32, 48), (100, 257), (130, 300), (257, 300), (130, 1000), (48, 32)}
    for n in tw.CASES:  # both element types of every case
        assert n.rsplit("_", 1)[0] + "_f32" in tw.CASES and n.rsplit("_", 1)[0] + "_f64" in tw.CASES
    A, _, _, y = tw.case_data("32x48k8s19_f64")
    x, info = tw.fsbl(A, y, S2, maxiter=5)  # reaching a cap is no error
    assert info["iterations"] == 5 and not info["converged"] and len(info["history"]) == 5


@pytest.mark.parametrize("name,solver,t", [("32x48k8s19_f64", "fsbl", 21), ("100x257k20s23_f64", "fsbl", 30), ("130x300k25s7_f64", "fsbl", 17)])
def test_warm_start_of_the_twin(name, solver, t):
    """running to pass t, then restarting from that α, reproduces the remaining history, and x to 1e-9"""
    A, _, _, y = tw.case_data(name)
    A = np.asarray(A, np.float64)
    x, info = tw.case_twin(name, solver)
    _, head = tw.fsbl(A, y, S2, maxiter=t)
    x2, tail = tw.fsbl(A, y, S2, alpha=head["alpha"])
    assert head["history"] + tail["history"] == info["history"] and head["iterations"] + tail["iterations"] == info["iterations"]
    assert np.array_equal(np.isfinite(tail["alpha"]), np.isfinite(info["alpha"]))
    assert _rel(x2, x) <= 1e-9


def test_zero_column_of_the_twin():
    A, _, _, y = tw.case_data("32x48_f64")
    Z = np.array(A)
    Z[:, 5] = 0.0
    for fn in (tw.fsbl, tw.rmps):
        x, info = fn(Z, y, S2)
        assert x[5] == 0.0 and info["alpha"][5] == np.inf and np.all(np.isfinite(x))
        assert all(i != 5 for _, i in info["history"])


def test_refusals_mirror_the_library(cs):
    """the twin and the package refuse the same arguments (the package before it touches a device)"""
    A, _, _, y = tw.case_data("32x48_f64")
    M, N = A.shape
    for twf, csf, caps in ((tw.fsbl, cs.fsbl, ("maxiter",)), (tw.rmps, cs.rmps, ("maxiter", "maxiter_acquisition", "maxiter_deletion"))):
        bads = [dict(sigma2=0.0), dict(sigma2=-1.0), dict(sigma2=float("inf")), dict(sigma2=float("nan")), dict(min_increase=-1.0),
                dict(min_increase=float("nan"))] + [{c: 0} for c in caps]
        for bad in bads:
            kw = dict(sigma2=1e-4)
            kw.update(bad)
            s2 = kw.pop("sigma2")
            with pytest.raises(ValueError):
                twf(A, y, s2, **kw)
            with pytest.raises(ValueError):
                csf(A, y, s2, **kw)
        for a in (np.zeros(N), -np.ones(N), np.r_[np.full(N - 1, np.inf), np.nan], np.r_[np.full(N - 1, np.inf), -np.inf], np.full(N - 1, np.inf)):
            with pytest.raises(ValueError):
                twf(A, y, 1e-4, alpha=a)
            with pytest.raises(ValueError):
                csf(A, y, 1e-4, alpha=a)
        with pytest.raises(ValueError):
            csf(A, y[:-1], 1e-4)
        for fn in (lambda S: twf(A, y, S), lambda S: csf(A, y, S)):
            with pytest.raises(NotImplementedError):
                fn(1e-4 * np.eye(M))
    for s2 in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            cs.FSBL(A, y, s2)
    with pytest.raises(NotImplementedError):
        cs.FSBL(A, y, 1e-4 * np.eye(M))
    with pytest.raises(NotImplementedError) as e:  # the reference's rmps(A, b, Val(true), ...)
        cs.rmps(A, y, True)
    assert "σ²-optimising" in str(e.value)
