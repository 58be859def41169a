"""CPU tests of the dictionary analysis boundary -- csmp_colnorms and csmp_cumbabel in the header, the ctypes table, the package, the
Julia wrapper and the library's exports agree -- and of the numpy twin (tests/analysis_twin.py) the GPU parity tests measure against."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_twin as tw  # noqa: E402
from test_julia_binding import c_class, c_prototypes, jl_class, julia_ccalls  # noqa: E402

PROTOTYPES = {
    "csmp_colnorms": "int csmp_colnorms(csmp_ctx *ctx, double *norms, int out_loc);",
    "csmp_cumbabel": "int csmp_cumbabel(csmp_ctx *ctx, int64_t k, int normalize, double *mu, int64_t *pair);",
}


def _params(proto):
    inner = proto[proto.index("(") + 1:proto.rindex(")")]
    return [c_class(p.strip()) for p in inner.split(",")]


def _comment(src, name):
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*(?:#define [A-Z_]+ \d+\s*)?int %s\(" % name, src, flags=re.S)
    assert m, f"{name} has no comment in front of it"
    return re.sub(r"\s+", " ", m.group(1))


def test_header_declares_the_prototypes():
    src = open(os.path.join(ROOT, "include", "csmp.h")).read()
    flat = re.sub(r"\s+", " ", src)
    for name, proto in PROTOTYPES.items():
        assert proto in flat, name
        assert c_prototypes()[name] == ("i32", _params(proto))
    assert re.search(r"^#define CSMP_BABEL_KMAX 1024$", src, flags=re.M)
    doc = _comment(src, "csmp_colnorms")
    for need in ("src/util.jl:2", "CSMP_HOST", "CSMP_DEVICE", "zero column", "CSMP_EINVAL", "CSMP_ESTATE", "CSMP_HOST_STREAMED", "CSMP_ENOMEM"):
        assert need in doc, need
    doc = _comment(src, "csmp_cumbabel")
    for need in ("src/util.jl:96-115", "self entry", "normalize = 1", "zero column", "tie-break", "lowest i", "lowest j", "(-1, -1)", "CSMP_EINVAL",
                 "CSMP_ERANGE", "CSMP_BABEL_KMAX", "CSMP_ESTATE", "CSMP_HOST_STREAMED", "CSMP_ENOMEM"):
        assert need in doc, need


def test_binding_table_binds_them(cs):
    C = ctypes
    ctype = {"i32": C.c_int, "i64": C.c_int64, "f64": C.c_double}
    for name, proto in PROTOTYPES.items():
        res, args = cs._lib.SIGNATURES[name]
        assert res is C.c_int
        want = _params(proto)
        assert len(args) == len(want)
        for pos, (a, c) in enumerate(zip(args, want)):
            assert (a is C.c_void_p) if c.startswith("ptr") else (a is ctype[c]), (name, pos, a, c)
    assert cs._lib.BABEL_KMAX == 1024
    assert callable(cs.Context.colnorms) and callable(cs.Context.cumbabel)


def test_package_exports(cs):
    for name in ("colnorms", "cumbabel", "babel", "coherence"):
        assert name in cs.__all__ and callable(getattr(cs, name)), name
    A = np.asarray(tw.random_dictionary(16, 24, "f64"))
    for k in (0, -1, 25, 2.0):  # ValueError before the library is reached (no GPU here)
        with pytest.raises(ValueError):
            cs.cumbabel(A, k)
        with pytest.raises(ValueError):
            cs.babel(A, k)
    with pytest.raises(ValueError):
        cs.cumbabel(np.zeros((4, 2000)), 1025)
    with pytest.raises(ValueError):
        cs.coherence(A, normalize=2)


def test_julia_wrapper_calls_them():
    src = open(os.path.join(ROOT, "compressedsensing.jl_amd", "julia", "CompressedSensingAMD.jl")).read()
    for fn in ("colnorms", "cumbabel", "babel", "coherence"):
        assert re.search(r"^(?:function )?%s\(A::MatOrDict" % fn, src, flags=re.M), fn
    assert "Int(pair[1]) + 1, Int(pair[2]) + 1" in src  # the pair is 1-based on the Julia side
    for name, proto in PROTOTYPES.items():
        calls = [parts for _, parts in julia_ccalls() if re.fullmatch(r"\(\s*:%s\s*,\s*libcsmp\s*\)" % name, parts[0])]
        assert len(calls) == 1, name
        parts = calls[0]
        assert jl_class(parts[1]) == "i32"
        types = [jl_class(t) for t in parts[2].strip()[1:-1].split(",")]
        want = _params(proto)
        assert len(types) == len(want) == len(parts) - 3
        for pos, (j, c) in enumerate(zip(types, want)):
            assert j == c or (j.startswith("ptr") and c.startswith("ptr") and "void" in (j[4:], c[4:])), (name, pos, j, c)


def test_library_exports_the_symbols(cs):
    L = ctypes.CDLL(cs.LIB_PATH)
    for name in PROTOTYPES:
        assert hasattr(L, name), name


# ------------------------------------------------------------------------------------------ the twin, pinned by properties
def _hadamard(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def test_twin_orthonormal_basis_gives_zero():
    Q, _ = np.linalg.qr(np.random.default_rng(0).standard_normal((24, 24)))
    mu = tw.cumbabel(Q, 23)
    assert np.all(mu <= tw.tolerance(Q, mu))
    assert np.array_equal(tw.cumbabel(np.eye(16), 16), np.zeros(16)) and tw.pair(np.eye(16)) == (0, 1)
    assert tw.pair(np.ones((16, 1))) == (-1, -1) and tw.cumbabel(np.ones((16, 1)), 1)[0] == 0.0


def test_twin_identity_beside_hadamard():
    M = 64
    A = np.hstack([np.eye(M), _hadamard(M) / np.sqrt(M)])
    assert tw.coherence(A) == 0.125 and tw.coherence(A, normalize=True) == 0.125  # exactly 1/√M
    assert tw.pair(A) == (0, 64)
    mu = tw.cumbabel(A, 64)
    assert np.array_equal(mu, 0.125 * np.arange(1, 65))  # a column meets the 64 of the other basis at 1/√M each


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twin_monotone_and_self_zero(seed):
    A = np.asarray(tw.random_dictionary(20, 33, "f64", seed))
    N = A.shape[1]
    for normalize in (False, True):
        mu = tw.cumbabel(A, N, normalize)
        assert np.all(np.diff(mu) >= 0) and np.all(mu <= np.arange(1, N + 1) * mu[0] * (1 + 1e-15))
        assert mu[N - 1] == tw.cumbabel(A, N - 1, normalize)[N - 2]  # the self entry is the zero added last
        assert tw.babel(A, 5, normalize) == mu[4] and tw.coherence(A, normalize) == mu[0]
        i, j = tw.pair(A, normalize)
        assert i < j and tw.gram_abs(A, normalize)[i, j] == mu[0]
    assert tw.coherence(A, True) <= 1.0 + 1e-15


def test_twin_duplicated_column():
    A = np.array(tw.random_dictionary(20, 33, "f64", 3))
    A[:, 29] = A[:, 4]
    assert tw.pair(A) == (4, 29) and tw.pair(A, True) == (4, 29)
    n2 = float(A[:, 4] @ A[:, 4])
    assert abs(tw.coherence(A) - n2) <= 4 * tw.gamma(20) * n2
    assert abs(tw.coherence(A, True) - 1.0) <= 4 * tw.gamma(28)
    A[:, 7] = 0.0  # a zero column contributes nothing, normalised or not
    G = tw.gram_abs(A, True)
    assert np.isfinite(G).all() and not G[7].any() and not G[:, 7].any()


@pytest.mark.parametrize("seed", [0, 1])
def test_twin_agrees_with_the_loop_over_columns(seed):
    A = np.asarray(tw.random_dictionary(50, 70, "f32", seed))
    for k in (1, 9, 70):
        mu, ref = tw.cumbabel(A, k), tw.cumbabel_by_columns(A, k)
        assert np.all(np.abs(mu - ref) <= tw.tolerance(A, ref)), k


def test_integer_dictionaries_tie_where_planted():
    for M, N, dt in ((200, 130, "f32"), (64, 300, "f64")):
        A = tw.integer_dictionary(M, N, dt, 7, planted=True)
        assert tw.pair(A) == (3, 5) and tw.coherence(A) == 4.0 * M
        G = tw.gram_abs(A)
        assert np.count_nonzero(np.triu(G, 1) == 4.0 * M) >= 6  # several pairs tie
        assert np.array_equal(tw.cumbabel(A, 9), tw.cumbabel_by_columns(A, 9))  # exact arithmetic: no order matters
        B = tw.integer_dictionary(M, N, dt, 7, planted=False)
        assert tw.coherence(B) < 4.0 * M
