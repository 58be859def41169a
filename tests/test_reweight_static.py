"""CPU tests of the reweighted l1 path: the numpy twin (tests/reweight_twin.py) has the reference's own property
(test/basispursuit.jl:18-36: the reweighted solves return the planted support), its two restatements of ard_weights! agree far inside
the tolerance the GPU test uses, its refusals are the library's, and the bindings carry the header's constants."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ista_twin as tw  # noqa: E402
import reweight_twin as rt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "csmp.h")


@pytest.mark.parametrize("accel", [False, True], ids=["ista", "fista"])
@pytest.mark.parametrize("scheme", ["candes", "ard"])
@pytest.mark.parametrize("shape", rt.SOLVE_SHAPES)
def test_reweighted_solves_return_the_planted_support(shape, scheme, accel):
    """λ = 2e-2, stepsize(A), 1024 inner iterations, ε = 1e-2, 8 outer solves"""
    _, x0, _, _, _ = tw.case_data(shape)
    x, w, done, h, _ = rt.solve_twin(shape, scheme, accel)
    print("step norms:", " ".join(f"{v:.2e}" for v in h))
    assert done == 8 and len(h) == 7
    assert np.array_equal(np.flatnonzero(x), np.flatnonzero(x0))
    assert h[-1] < 1e-6 * h[0]  # (the step norms fall by roughly 100 x per outer solve)
    assert np.all(np.isfinite(w)) and np.all(w > 0)


@pytest.mark.parametrize("scheme", ["candes", "ard"])
def test_early_exit_instance(scheme):
    """the instance the GPU test of the early exit stands on: the threshold sqrt(h[2] h[3]) is a factor of 5 from either neighbour"""
    h = rt.solve_twin("32x48_f64", scheme, False)[3]
    assert h[2] / h[3] >= 25
    md = float(np.sqrt(h[2] * h[3]))
    x, _, done, h2, _ = rt.solve_twin("32x48_f64", scheme, False, md)
    assert done == 5 and h2 == h[:4]
    assert np.array_equal(np.flatnonzero(x), np.flatnonzero(tw.case_data("32x48_f64")[1]))


@pytest.mark.parametrize("ones", [True, False], ids=["ones", "random"])
@pytest.mark.parametrize("it", [1, 8])
@pytest.mark.parametrize("name", list(rt.WEIGHT_CASES))
def test_the_two_restatements_agree(name, it, ones):
    """ard_direct (the M x M matrix K) against ard_support (the k x k matrix) within a TENTH of the tolerance of the GPU test, on
    every weight case of it: the tolerance is not set by one formulation's luck"""
    A, x, w_in = rt.weight_case(name)
    ws, bound, kappa = rt.weight_twin(name, it, ones)
    wd = rt.ard_direct(A, x, None if ones else w_in, rt.EPS, it)
    err = np.abs(ws ** 2 - wd ** 2)
    print(f"kappa = {kappa:.2e}  max |Δw²| = {err.max():.2e}  max |Δw²| / bound = {np.max(err / bound):.2e}")
    assert 1.0 <= kappa <= 1e3
    assert np.all(err <= 0.1 * bound)


def test_k0_and_first_iteration_formulas():
    A, x, _ = rt.weight_case("64x256_f64_k0")
    assert not x.any()
    n = np.linalg.norm(A.astype(np.float64), axis=0)
    assert np.allclose(rt.ard_support(A, x, None, rt.EPS, 8), n / np.sqrt(rt.EPS), rtol=1e-14)
    # atoms of the support: a_i' K^-1 a_i = 1/d_i - eps (H^-1)_ii / d_i^2 -- a third route to the same numbers
    A, x, w_in = rt.weight_case("32x48_f64_k3")
    S = np.flatnonzero(x)
    A64 = A.astype(np.float64)
    d = np.abs(x[S]) / w_in[S]
    H = np.diag(rt.EPS / d) + A64[:, S].T @ A64[:, S]
    third = np.sqrt(1.0 / d - rt.EPS * np.diag(np.linalg.inv(H)) / d ** 2)
    assert np.allclose(rt.ard_support(A, x, w_in, rt.EPS, 1)[S], third, rtol=1e-10)


def test_refusals_of_the_twin_mirror_the_library():
    A, x, w_in = rt.weight_case("32x48_f64_k3")
    N = A.shape[1]
    for fn in (rt.ard_direct, rt.ard_support):
        for j in (0, N - 1):
            w = np.ones(N)
            w[j] = 0.0
            with pytest.raises(ValueError, match="zero"):  # CSMP_EINVAL
                fn(A, x, w)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                fn(A, x, np.where(np.arange(N) == 3, bad, 1.0))
        for bad in (0.0, -1e-2, float("nan"), float("inf")):
            with pytest.raises(ValueError):  # CSMP_EINVAL
                fn(A, x, None, bad)
        with pytest.raises(ValueError):
            fn(A, x, None, rt.EPS, 0)
        x33 = np.zeros(N)
        x33[:33] = 1.0
        with pytest.raises(IndexError):  # CSMP_ERANGE: 33 non-zeros at M = 32
            fn(A, x33)
        x33[32] = 0.0
        assert np.all(np.isfinite(fn(A, x33, None, rt.EPS, 1)))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            rt.candes_weights(x, bad)
    with pytest.raises(ValueError):
        rt.candes_weights(np.array([1.0, float("nan")]), 1e-2)
    _, _, b, alpha, _ = tw.case_data("32x48_f64")
    for kw in ({"eps": 0.0}, {"ard_iter": 0}, {"maxiter": 0}, {"min_decrease": -1.0}, {"min_decrease": float("nan")}, {"scheme": 2}):
        args = {"scheme": rt.ARD, "eps": rt.EPS, "ard_iter": 8, "maxiter": 2, "min_decrease": 0.0, **kw}
        with pytest.raises(ValueError):
            rt.reweighted(A, b, rt.LAMBDA, args["scheme"], args["eps"], args["ard_iter"], args["maxiter"], args["min_decrease"], 4, alpha)


def test_candes_twin_matches_the_formula():
    x = np.array([0.0, -2.0, 0.5, 1e-300])
    assert np.array_equal(rt.candes_weights(x, 1e-2), 1.0 / (np.abs(x) + 1e-2))


def test_header_bindings_and_documents_carry_the_exports():
    hdr = open(HDR).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CSMP_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", hdr)}
    assert consts["CSMP_ARD_KMAX"] == rt.ARD_KMAX >= 1024
    assert (consts["CSMP_REWEIGHT_CANDES"], consts["CSMP_REWEIGHT_ARD"]) == (rt.CANDES, rt.ARD) == (0, 1)
    for name in ("csmp_ard_weights", "csmp_ista_reweighted"):
        assert re.search(r"\bint %s\(csmp_ctx \*ctx," % name, hdr), name
    lib = open(os.path.join(ROOT, "compressedsensing.jl_amd", "_lib.py")).read()
    assert re.search(r"^ARD_KMAX = %d\b" % rt.ARD_KMAX, lib, flags=re.M) and '"csmp_ard_weights"' in lib and '"csmp_ista_reweighted"' in lib
    jl = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    for sym in (":csmp_ard_weights", ":csmp_ista_reweighted", "candes_weights!", "ard_weights!", "ista_candes", "ista_ard"):
        assert sym in jl, sym
    for doc, words in (("DESIGN.md", ("k_ard_forms", "ista_ard")), ("README.md", ("ista_candes", "ista_ard")),
                       ("INTEGRATION.md", ("csmp_ard_weights", "csmp_ista_reweighted"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
    # the kernels and the host code live where the build expects them, and the outer loop lives in the library
    hip = open(os.path.join(ROOT, "compressedsensing.jl_amd", "csrc", "csmp.hip")).read()
    assert '#include "csmp_reweight.hpp"' in hip and '#include "host/reweight.hpp"' in hip
