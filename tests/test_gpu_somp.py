"""GPU tests (pytest -m gpu) of csmp_somp: simultaneous OMP, ONE support for all columns of B, on the shared pass.  The reference is the
numpy twin (tests/somp_twin.py, checked on the CPU by tests/test_somp_static.py): order and support identical -- no pick of any case is
a near-tie in the twin --, coefficients and residual norms to 1e-6 of the largest reference entry.  Beside the parity: the passes a
step takes, the finish beyond 256 columns, a dictionary without a shared pass, one column against csmp_omp, equal columns, the eps
stop, the same bits under every schedule, the refusals at the ABI and failed allocations."""
import ctypes
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import somp_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-6


@pytest.fixture
def D(cs):
    """dictionaries of ONE test, closed when it ends"""
    made = []

    def make(A, **kw):
        d = cs.Dictionary(A, **kw)
        made.append(d)
        return d
    yield make
    for d in made:
        d.close()


def run(d, B, k, eps=0.0, p=1, **tunes):
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return d.ctx.somp(B, k, eps, p)
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2]["order"], b[2]["order"])
            and np.array_equal(a[2]["resnorm"], b[2]["resnorm"]) and a[2]["steps"] == b[2]["steps"] and a[2]["passes"] == b[2]["passes"])


def check(got, t, what):
    idx, val, info = got
    print(what, "steps", info["steps"], "passes", info["passes"],
          "coef err", float(np.max(np.abs(val - t.X))) / float(np.max(np.abs(t.X))) if val.shape == t.X.shape else None,
          "resnorm err", float(np.max(np.abs(info["resnorm"] - t.resnorm))) / float(np.max(t.resnorm)))
    assert np.array_equal(info["order"], t.order), what
    assert np.array_equal(idx, t.support), what
    assert info["steps"] == len(t.order)
    assert val.shape == t.X.shape
    assert np.max(np.abs(val - t.X)) <= RTOL * np.max(np.abs(t.X)), what
    assert np.max(np.abs(info["resnorm"] - t.resnorm)) <= RTOL * np.max(t.resnorm), what


@pytest.mark.parametrize("shape", list(tw.SHAPES))
def test_parity_with_the_twin(cs, D, shape):
    A, B = tw.shape_data(shape)
    d = D(A)
    cfg = d.ctx.sweep_config()
    wide = 8 if A.dtype == np.float32 else 4
    assert cfg["group_max"] == 4 and cfg["group_wide"] == wide
    for nsig in tw.NSIGS:
        for p in tw.PS:
            name = f"{shape}-{nsig}-p{p}"
            got = d.ctx.somp(tw.columns(B, nsig), tw.K, 0.0, p)
            check(got, tw.reference(name), name)
            assert got[2]["passes"] == got[2]["steps"] * -(-nsig // wide), name   # the shared pass, not one sweep per column
    # the public function: SparseVectors that all carry the same nzind
    xs, info = cs.somp(d, tw.columns(B, 9), tw.K, return_info=True)
    ref = d.ctx.somp(tw.columns(B, 9), tw.K, float(np.finfo(A.dtype).eps), 1)
    assert len(xs) == 9 and all(np.array_equal(x.nzind, ref[0]) and np.array_equal(x.nzval, ref[1][:, s]) for s, x in enumerate(xs))
    assert np.array_equal(info["order"], ref[2]["order"]) and info["steps"] == tw.K and info["passes"] == ref[2]["passes"]


def test_long_support(cs, D):
    """k = 260: launch_finish changes scheme beyond 256 columns, k_somp_solve does not"""
    shape, nsig, k = tw.LONG
    A, B = tw.shape_data(shape)
    d = D(A)
    got = d.ctx.somp(tw.columns(B, nsig), k, 0.0, 1)
    check(got, tw.reference("long"), "long")
    assert got[2]["steps"] == k and got[2]["passes"] == k


def test_dictionary_without_a_shared_pass(cs, D):
    """a column longer than the LDS holds: the sweeps are phased, one per column and step"""
    M, N, dtype, seed, nsig, k = tw.PHASED
    A, B = tw.planted(M, N, dtype, seed, nsig)
    d = D(A)
    assert d.ctx.sweep_config()["group_max"] == 0
    got = d.ctx.somp(B, k, 0.0, 1)
    check(got, tw.reference("phased"), "phased")
    assert got[2]["passes"] == got[2]["steps"] * nsig == k * nsig


def test_one_column_is_omp(cs, D):
    A, B = tw.shape_data("f32")
    d = D(A)
    b = B[:, 0]
    idx, val, order = d.ctx.omp(b, tw.K, 0.0)
    for p in tw.PS:
        got = d.ctx.somp(tw.columns(B, 1), tw.K, 0.0, p)
        assert np.array_equal(got[0], idx) and np.array_equal(got[2]["order"], order), p
        assert np.max(np.abs(got[1][:, 0] - val)) <= RTOL * np.max(np.abs(val)), p
    zero = np.zeros((A.shape[0], 1), order="F")
    zidx, zval, zorder = d.ctx.omp(zero[:, 0], tw.K, 0.0)
    got = d.ctx.somp(zero, tw.K, 0.0, 1)
    assert np.array_equal(got[0], zidx) and np.array_equal(got[2]["order"], zorder) and np.array_equal(got[1][:, 0], zval)
    assert np.all(got[2]["resnorm"] == 0.0)


def test_copies(cs, D):
    """B = [b b b]: omp(b)'s picks, and three columns that are equal bit for bit"""
    A, B3 = tw.copies()
    d = D(A)
    _, _, order = d.ctx.omp(B3[:, 0], tw.K, 0.0)
    got = d.ctx.somp(B3, tw.K, 0.0, 1)
    check(got, tw.reference("copies"), "copies")
    assert np.array_equal(got[2]["order"], order)
    assert np.array_equal(got[1][:, 0], got[1][:, 1]) and np.array_equal(got[1][:, 0], got[1][:, 2])
    assert got[2]["resnorm"][0] == got[2]["resnorm"][1] == got[2]["resnorm"][2]


def test_eps_stop(cs, D):
    shape, nsig, p = tw.EPS_CASE
    full = tw.reference(f"{shape}-{nsig}-p{p}")
    eps = 0.5 * (full.hist[5] + full.hist[6])
    A, B = tw.shape_data(shape)
    d = D(A)
    t = tw.somp(A, tw.columns(B, nsig), eps, tw.K, p)
    assert len(t.order) == 7
    got = d.ctx.somp(tw.columns(B, nsig), tw.K, eps, p)
    check(got, t, "eps")
    assert got[2]["steps"] == 7 and got[2]["passes"] == 8   # (the pass of the step that found ||R||_F below eps ran)
    assert np.isclose(np.linalg.norm(got[2]["resnorm"]), full.hist[6], rtol=RTOL)


def test_same_bits_everywhere(cs, D):
    import torch
    A, B = tw.shape_data("f32")
    d = D(A)
    for nsig, p in ((17, 1), (9, 2)):
        Bn = tw.columns(B, nsig)
        first = d.ctx.somp(Bn, tw.K, 0.0, p)
        check(first, tw.reference(f"f32-{nsig}-p{p}"), "first")
        assert same(d.ctx.somp(Bn, tw.K, 0.0, p), first)
        Bt = torch.from_numpy(np.array(Bn.T, order="C")).to("cuda").T
        assert Bt.shape == Bn.shape and Bt.stride() == (1, Bn.shape[0])
        assert same(d.ctx.somp_device(Bt, tw.K, 0.0, p), first)
        for tunes in ({"pipelines": 1}, {"pipelines": 2}, {"pipelines": 3}):
            assert same(run(d, Bn, tw.K, 0.0, p, **tunes), first), tunes
        for tunes in ({"group_max": 1}, {"group_max": 2}, {"group_wide": 1}):   # other chunks: more passes, the same numbers
            got = run(d, Bn, tw.K, 0.0, p, **tunes)
            width = {"group_max": tunes.get("group_max"), "group_wide": 4}[next(iter(tunes))]
            assert got[2]["passes"] == tw.K * -(-nsig // width), tunes
            got[2]["passes"] = first[2]["passes"]
            assert same(got, first), tunes
        assert same(d.ctx.somp(Bn, tw.K, 0.0, p), first)


# ---- the ABI
OK, EINVAL, ERANGE, ESTATE = 0, -1, -3, -5
AM, AN, ANSIG, AK = 64, 256, 3, 4
_VALID = dict(ldB=AM, k=AK, nsig=ANSIG, eps=0.0, p=1)
_ARG_CASES = [
    ("no_dictionary", dict(no_dict=True), ESTATE), ("ldB_lt_M", dict(ldB=AM - 1), EINVAL), ("p_0", dict(p=0), EINVAL), ("p_3", dict(p=3), EINVAL),
    ("k_0", dict(k=0), EINVAL), ("eps_neg", dict(eps=-1.0), EINVAL), ("eps_nan", dict(eps=float("nan")), EINVAL),
    ("k_gt_M", dict(k=AM + 1), ERANGE), ("nsig_0", dict(nsig=0), OK),
]


@pytest.fixture(scope="module")
def contexts(cs):
    A, _, _ = cs.sparse_data(n=AM, m=AN, k=AK, rng=5, dtype=np.float32)
    with_dict = cs.Dictionary(A)
    bare = cs._lib.Context(0)
    yield with_dict.ctx, bare
    bare.close()
    with_dict.close()


def _call(L, ctx, a):
    nsig, k = a["nsig"], a["k"]
    rng = np.random.default_rng(11)
    B = np.asfortranarray(rng.standard_normal((AM, max(nsig, 1))))
    kk = max(k, 1)
    idx, order = np.full(kk, 5, np.int64), np.full(kk, 5, np.int64)
    val = np.full((kk, max(nsig, 1)), 5.0, np.float64, order="F")
    res = np.full(max(nsig, 1), 5.0)
    nnz, passes = L.i64(5), L.i64(5)
    rc = L.lib().csmp_somp(ctx._h, L.ptr(B), 1, L.i64(a["ldB"]), L.i64(nsig), 0, L.i64(k), ctypes.c_double(a["eps"]), a["p"], L.ptr(idx),
                           L.ptr(val), L.i64(kk), ctypes.byref(nnz), L.ptr(order), L.ptr(res), ctypes.byref(passes), 0)
    return rc, idx, val, order, res, nnz.value, passes.value


@pytest.mark.parametrize("over,want", [pytest.param(o, w, id=name) for name, o, w in _ARG_CASES])
def test_arguments(cs, contexts, over, want):
    L = cs._lib
    with_dict, bare = contexts
    ctx = bare if over.get("no_dict") else with_dict
    rc, idx, val, order, res, nnz, passes = _call(L, ctx, dict(_VALID, **over))
    assert rc == want
    if rc != OK or over.get("nsig") == 0:  # nothing was written
        assert np.all(idx == 5) and np.all(val == 5.0) and np.all(order == 5) and np.all(res == 5.0) and nnz == 5 and passes == 5
    if ctx is with_dict:  # the context is still good for a valid call
        rc, idx, val, order, res, nnz, passes = _call(L, ctx, _VALID)
        assert rc == OK and nnz == AK and passes == AK and np.all(np.diff(idx) > 0) and sorted(order) == list(idx)


def test_null_outputs_are_allowed(cs, contexts):
    L = cs._lib
    ctx, _ = contexts
    rng = np.random.default_rng(11)
    B = np.asfortranarray(rng.standard_normal((AM, ANSIG)))
    idx, val, nnz = np.zeros(AK, np.int64), np.zeros((AK, ANSIG), order="F"), L.i64(0)
    rc = L.lib().csmp_somp(ctx._h, L.ptr(B), 1, L.i64(AM), L.i64(ANSIG), 0, L.i64(AK), ctypes.c_double(0.0), 2, L.ptr(idx), L.ptr(val), L.i64(AK),
                           ctypes.byref(nnz), None, None, None, 0)
    assert rc == OK and nnz.value == AK
    want = ctx.somp(B, AK, 0.0, 2)
    assert np.array_equal(idx, want[0]) and np.array_equal(val, want[1])


def test_every_allocation_may_fail(cs):
    """fail_alloc = n makes the n-th device allocation from now fail for real (the hook of tests/test_gpu_mp_batch.py).  For every n
    until the call goes through twice in a row: a failing call returns a status, and the same context then returns the clean bits."""
    L = cs._lib
    M, N, dtype, seed, nsig, k = tw.ALLOC
    A, B = tw.planted(M, N, dtype, seed, nsig)
    gc.collect()
    base = L.live_resources()
    clean = cs.Dictionary(A)
    assert clean.ctx.sweep_config()["group_wide"] == 8
    want = clean.ctx.somp(B, k, 0.0, 1)
    check(want, tw.reference("alloc"), "alloc")
    clean.close()
    n, seen_ok, failed = 0, 0, 0
    while seen_ok < 2 and n < 500:
        n += 1
        d = cs.Dictionary(A)
        d.ctx.tune("fail_alloc", n)
        try:
            got = d.ctx.somp(B, k, 0.0, 1)
            assert same(got, want), (n, "the call went through with a result of its own")
            seen_ok += 1
        except cs.CsmpError as e:
            seen_ok = 0
            failed += 1
            assert e.code in (L.EHIP, L.ENOMEM), (n, e.code, str(e))
        d.ctx.tune("fail_alloc", 0)
        assert same(d.ctx.somp(B, k, 0.0, 1), want), (n, "after the failed call")
        d.close()
    assert n < 500 and failed >= 10, (n, failed)   # (the slot's buffers and the call's thirteen arrays at the least)
    gc.collect()
    assert L.live_resources() == base
