"""The return code of every batch entry point for a table of bad inputs.

Each case changes one argument of an otherwise valid call (or drops the dictionary) and pins the code the C ABI returns.  The codes
include the entry points' differences: csmp_omp_batch_mfma refuses nsig = 0, the others return CSMP_OK for it; fr_batch checks its
tolerances for NaN only; sp_batch has no b_loc / out_loc and checks 2k > M after the dictionary."""
import ctypes as C

import numpy as np
import pytest

M, N, NSIG, K, L_GOMP = 64, 256, 3, 4, 2

# entry -> the arguments that make a valid call; a case overrides some of them
_VALID = {
    "omp_batch": dict(b_loc=0, out_loc=0, ldB=M, dtype=1, k=K, nsig=NSIG, eps=1e-6),
    "omp_batch_screened": dict(b_loc=0, out_loc=0, ldB=M, dtype=1, k=K, nsig=NSIG, eps=1e-6),
    "fr_batch": dict(b_loc=0, out_loc=0, ldB=M, dtype=1, k=K, nsig=NSIG, eps=0.0, min_delta=0.0),
    "gomp_batch": dict(b_loc=0, out_loc=0, ldB=M, dtype=1, k=K, nsig=NSIG, eps=1e-6, l=L_GOMP),
    "sp_batch": dict(ldB=M, dtype=1, k=K, nsig=NSIG, eps=1e-12),
    "omp_batch_mfma": dict(b_loc=0, out_loc=0, ldB=M, dtype=1, k=K, nsig=NSIG, eps=1e-6),
}

OK, EINVAL, ERANGE, ESTATE = 0, -1, -3, -5
nan = float("nan")

# (case name, overrides, {entry: code}); "*" is every entry the case applies to (sp_batch has no b_loc / out_loc)
_CASES = [
    ("b_loc", dict(b_loc=7), {"*": EINVAL, "sp_batch": None}),
    ("out_loc", dict(out_loc=-1), {"*": EINVAL, "sp_batch": None}),
    ("null_B", dict(null_B=True), {"*": EINVAL}),
    ("ldB_lt_M", dict(ldB=M - 1), {"*": EINVAL}),
    ("dtype", dict(dtype=5), {"*": EINVAL}),
    ("k_0", dict(k=0), {"*": EINVAL}),
    ("nsig_0", dict(nsig=0), {"*": OK, "omp_batch_mfma": EINVAL}),
    ("nsig_neg", dict(nsig=-1), {"*": EINVAL}),
    ("eps_neg", dict(eps=-1.0), {"*": EINVAL, "fr_batch": None, "sp_batch": None}),
    ("eps_nan", dict(eps=nan), {"*": EINVAL, "sp_batch": None}),
    ("min_delta_nan", dict(min_delta=nan), {"fr_batch": EINVAL}),
    ("l_gt_k", dict(l=K + 1), {"gomp_batch": EINVAL}),
    ("l_0", dict(l=0), {"gomp_batch": EINVAL}),
    ("sp_2k_gt_M", dict(k=M // 2 + 1), {"sp_batch": ERANGE}),
    ("no_dictionary", dict(no_dict=True), {"*": ESTATE}),
    ("no_dictionary_k_0", dict(no_dict=True, k=0), {"*": EINVAL}),
    ("no_dictionary_sp_2k_gt_M", dict(no_dict=True, k=M // 2 + 1), {"sp_batch": ESTATE}),
]


def _table():
    for case, over, codes in _CASES:
        for entry in _VALID:
            want = codes.get(entry, codes.get("*"))
            if want is not None:
                yield pytest.param(entry, over, want, id=f"{entry}-{case}")


@pytest.fixture(scope="module")
def contexts(cs):
    A, _, _ = cs.sparse_data(n=M, m=N, k=K, rng=5, dtype=np.float32)
    with_dict = cs.Dictionary(A)
    bare = cs._lib.Context(0)
    yield with_dict.ctx, bare
    bare.close()
    with_dict.close()


def _call(L, ctx, entry, a):
    nsig, k = a["nsig"], a["k"]
    rng = np.random.default_rng(11)
    B = np.asfortranarray(rng.standard_normal((M, max(nsig, 1))))
    idx = np.zeros((max(k, 1), max(nsig, 1)), np.int64, order="F")
    val = np.zeros((max(k, 1), max(nsig, 1)), np.float64, order="F")
    nnz = np.zeros(max(nsig, 1), np.int64)
    its = np.zeros(max(nsig, 1), np.int64)
    pB = None if a.get("null_B") else L.ptr(B)
    h, lib = ctx._h, L.lib()
    i64, d = L.i64, C.c_double
    if entry in ("omp_batch", "omp_batch_screened", "omp_batch_mfma"):
        fn = lib.csmp_omp_batch_mfma if entry == "omp_batch_mfma" else lib.csmp_omp_batch
        return fn(h, pB, a["dtype"], i64(a["ldB"]), i64(nsig), a["b_loc"], i64(k), d(a["eps"]), L.ptr(idx), L.ptr(val), L.ptr(nnz),
                  a["out_loc"])
    if entry == "fr_batch":
        return lib.csmp_fr_batch(h, pB, a["dtype"], i64(a["ldB"]), i64(nsig), a["b_loc"], i64(k), d(a["eps"]), d(a["min_delta"]),
                                 L.ptr(idx), L.ptr(val), L.ptr(nnz), a["out_loc"])
    if entry == "gomp_batch":
        return lib.csmp_gomp_batch(h, pB, a["dtype"], i64(a["ldB"]), i64(nsig), a["b_loc"], i64(a["l"]), i64(k), d(a["eps"]),
                                   L.ptr(idx), L.ptr(val), L.ptr(nnz), a["out_loc"])
    return lib.csmp_sp_batch(h, pB, a["dtype"], i64(a["ldB"]), i64(nsig), i64(k), d(a["eps"]), i64(-1), L.ptr(idx), L.ptr(val),
                             L.ptr(nnz), L.ptr(its))


@pytest.mark.gpu
@pytest.mark.parametrize("entry,over,want", list(_table()))
def test_batch_entry_return_code(cs, contexts, entry, over, want):
    L = cs._lib
    with_dict, bare = contexts
    ctx = bare if over.get("no_dict") else with_dict
    ctx.set_option("screened_sweep", 1 if entry == "omp_batch_screened" else 0)
    a = dict(_VALID[entry], **over)
    assert _call(L, ctx, entry, a) == want
    ctx.set_option("screened_sweep", 0)
    # the context is still good for a valid call
    if ctx is with_dict:
        assert _call(L, ctx, entry, _VALID[entry]) == OK
