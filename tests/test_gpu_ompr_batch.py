"""GPU tests (pytest -m gpu) of csmp_ompr_batch: ompr for every column of B, the update!s of a group's members in lockstep on shared
launches.  Every member keeps csmp_ompr's arithmetic -- the shared pass gives the single sweep's bits per member, the group kernels call
the single kernels' bodies on the member's own buffers, the host steps are OmprJob's -- so a batch must return the BITS of a caller's
loop over csmp_ompr on the same Dictionary: the support, the coefficients and the iteration count, whatever the batch size, the group
size and the order the slots are refilled in.  No tolerance against the single call anywhere; one signal per shape is held to the
oracle besides."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_shapes import close, gaussian, planted  # noqa: E402

pytestmark = pytest.mark.gpu

NSIGS = (2, 3, 8, 9, 17)
# (M, N, dtype, k): nchk = 2; ragged rows, k one past a kSwapChunk; more than one kResChunk, k^2 over several workgroups; k = 1; k = 16
SHAPES = {"256x1024_f32_k20": (256, 1024, np.float32, 20), "250x600_f64_k17": (250, 600, np.float64, 17),
          "640x1000_f32_k130": (640, 1000, np.float32, 130), "256x1024_f32_k1": (256, 1024, np.float32, 1),
          "256x1024_f32_k16": (256, 1024, np.float32, 16)}
OPTIONS = {"group1": {"group_max": 1}, "group1_narrow": {"group_max": 1, "group_wide": 1}, "group4_wide": {"group_max": 4},
           "group4_narrow": {"group_max": 4, "group_wide": 1}}
DELTA = 1e-9
_made = {}


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


def noisy(name):
    """(A, B, k): the shape's Gaussian dictionary and 17 planted signals with noise 0.3 and three more planted atoms than k -- the
    construction of test_ompr_exchange_guard_falls_back_to_the_qr_path; made once per shape, never changed"""
    if name not in _made:
        M, N, dtype, k = SHAPES[name]
        A = gaussian(M, N, dtype, 77 + M + k)
        B = np.asfortranarray(np.stack([planted(A, k + 3, 100 + s, noise=0.3) for s in range(max(NSIGS))], axis=1))
        _made[name] = (A, B, k)
    return _made[name]


def loop(d, B, k, delta=DELTA, maxiter=-1):
    """what a caller without the batch form writes: csmp_ompr column by column on the same Dictionary"""
    nsig = B.shape[1]
    ds = np.broadcast_to(np.asarray(delta, np.float64), (nsig,))
    return [d.ctx.ompr(np.ascontiguousarray(B[:, s]), k, float(ds[s]), maxiter) for s in range(nsig)]


def batch(d, B, k, delta=DELTA, maxiter=None, tunes=None, device=False):
    tunes = tunes or {}
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        if device:
            return d.ctx.ompr_batch_device(B, k, delta, maxiter)
        return d.ctx.ompr_batch(B, k, delta, maxiter)
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


def same(got, ref, cols=None):
    """the batch's columns against the single calls' results: indices, the BITS of the coefficients, the iteration counts"""
    idx, val, nnz, info = got
    cols = range(len(nnz)) if cols is None else cols                    # (the batch's column s is signal cols[s])
    for s, c in enumerate(cols):
        ri, rv, rit = ref[c]
        n = int(nnz[s])
        if n != len(ri) or not np.array_equal(idx[:n, s], ri) or not np.array_equal(val[:n, s], rv) or int(info["iterations"][s]) != rit:
            return False
    return True


# ------------------------------------------------------------------------------------------ 1. shapes and group sizes
@pytest.mark.parametrize("option", sorted(OPTIONS))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bits_of_the_loop(cs, oracle, D, name, option):
    A, B, k = noisy(name)
    d = D(A)
    cfg = d.ctx.sweep_config()
    # (a shared pass: the batch is not its own loop; Float32 dictionaries have the wide pass of two halves)
    assert cfg["group_max"] == 4 and cfg["group_wide"] == (8 if A.dtype == np.float32 else 4), cfg
    ref = loop(d, B, k)
    its = [r[2] for r in ref]
    print(f"{name} {option}: iterations of the single calls {its}")
    o = oracle.ompr(A, np.ascontiguousarray(B[:, 0]), k, DELTA)
    assert np.array_equal(ref[0][0], o[0]) and close(ref[0][1], o[1]) and ref[0][2] == o[2]
    # exchanges happened: an update! of a support of one atom cannot exchange -- the candidate's correlation is no larger than the
    # acquisition's, so the candidate itself is the smallest entry and the solve ends after its first update! -- beyond that, three
    assert max(its) >= (3 if k > 1 else 1), its
    for nsig in NSIGS:
        got = batch(d, np.asfortranarray(B[:, :nsig]), k, tunes=OPTIONS[option])
        assert not got[3]["solved_alone"].any(), (nsig, got[3])        # (else the single path would be compared with itself)
        assert same(got, ref), (nsig, got[3], its[:nsig])


# ------------------------------------------------------------------------------------------ 2. different end times
def mixed():
    """9 signals at 256 x 1024, k = 20: clean ones (k planted atoms, no noise to speak of), noisy ones, heavily noisy ones"""
    if "mixed" not in _made:
        A = noisy("256x1024_f32_k20")[0]
        cols = [planted(A, 20, 300 + s, noise=1e-7) if s % 3 == 0 else planted(A, 23 + s, 300 + s, noise=0.3 if s % 3 == 1 else 1.0) for s in range(9)]
        _made["mixed"] = np.asfortranarray(np.stack(cols, axis=1))
    return noisy("256x1024_f32_k20")[0], _made["mixed"], 20


def test_members_end_at_different_times(cs, D):
    A, B, k = mixed()
    d = D(A)
    ref = loop(d, B, k)
    its = [r[2] for r in ref]
    print(f"iterations of the single calls: {its}")
    assert len(set(its)) >= 3, its
    got = batch(d, B, k)
    assert same(got, ref) and not got[3]["solved_alone"].any(), (got[3], its)
    # reversed column order: other slots, another refill order, the same results
    rev = batch(d, np.asfortranarray(B[:, ::-1]), k)
    assert same(rev, ref, cols=range(8, -1, -1)), rev[3]
    # maxiter = 2 cuts the long solves
    ref2 = loop(d, B, k, maxiter=2)
    assert max(r[2] for r in ref2) == 2
    assert same(batch(d, B, k, maxiter=2), ref2)
    # one delta per signal, one of them large enough to end its signal after the first update!
    deltas = np.full(9, DELTA)
    deltas[4] = 1e3
    refd = loop(d, B, k, delta=deltas)
    assert refd[4][2] == 1 and its[4] > 1
    assert same(batch(d, B, k, delta=deltas), refd)


# ------------------------------------------------------------------------------------------ 3. the refresh inside a group
def test_refresh_in_lockstep(cs, D):
    """test_ompr_many_exchanges_on_a_coherent_dictionary's construction: more than kSwapRefresh = 32 accepted exchanges per solve"""
    M, N, k, mix, noise = 384, 3000, 150, 0.8, 3.0
    g = np.random.default_rng(6)
    sh = g.standard_normal((M, 1))
    A = g.standard_normal((M, N)) + mix * np.sqrt(M) * sh / np.linalg.norm(sh)
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    A = np.asfortranarray(A.astype(np.float32))
    cols = []
    for s in range(3):
        xs = cs.sparse_vector(N, k, rng=g)
        cols.append(cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, noise, rng=g))
    B = np.asfortranarray(np.stack(cols, axis=1))
    d = D(A)
    ref = loop(d, B, k, delta=0.0, maxiter=400)
    its = [r[2] for r in ref]
    print(f"iterations of the single calls: {its}")
    assert min(its) >= 33, its
    got = batch(d, B, k, delta=0.0, maxiter=400)
    print(f"solved alone: {got[3]['solved_alone']}")
    assert same(got, ref), got[3]
    assert not got[3]["solved_alone"].all()                              # (a coherent dictionary may refuse an exchange: not all of them)


# ------------------------------------------------------------------------------------------ 4. leaving the lockstep
def test_members_leave_the_lockstep(cs, D):
    A, Ball, k = noisy("256x1024_f32_k20")
    B = np.asfortranarray(Ball[:, :5])
    d = D(A)
    ref = loop(d, B, k)
    d.ctx.tune("swap_refuse", 1)
    try:
        hooked = loop(d, B, k)
        got = batch(d, B, k)
    finally:
        d.ctx.tune("swap_refuse", 0)
    assert got[3]["solved_alone"].all(), got[3]
    assert same(got, hooked)
    # (the QR path's coefficients are not the exchanges' bits: the supports and the iteration counts are)
    for s in range(5):
        n = int(got[2][s])
        assert np.array_equal(got[0][:n, s], ref[s][0]) and close(got[1][:n, s], ref[s][1]) and int(got[3]["iterations"][s]) == ref[s][2]
    again = batch(d, B, k)
    assert not again[3]["solved_alone"].any() and same(again, ref)       # the slots are clean


# ------------------------------------------------------------------------------------------ 5. locations
def test_locations_and_fallbacks(cs, D):
    import torch
    A, Ball, k = noisy("256x1024_f32_k20")
    M = A.shape[0]
    B = np.asfortranarray(Ball[:, :9])
    d = D(A)
    ref = loop(d, B, k)
    for dtype in (np.float32, np.float64):
        Bd = np.asfortranarray(B.astype(dtype))
        refd = ref if dtype is np.float64 else loop(d, Bd, k)
        assert same(batch(d, Bd, k), refd), dtype
        ld = M + 5                                                        # ldB > M
        T = torch.zeros((9, ld), dtype=torch.float32 if dtype is np.float32 else torch.float64, device="cuda")
        T[:, :M] = torch.from_numpy(np.ascontiguousarray(Bd.T)).cuda()
        Bt = T.t()[:M]                                                    # (M, 9) with stride (1, ld)
        assert Bt.stride() == (1, ld)
        got = batch(d, Bt, k, device=True)
        assert same(got, refd) and not got[3]["solved_alone"].any(), dtype
    # a lone signal, and the screened sweeps: the loop's results
    one = batch(d, np.asfortranarray(B[:, :1]), k)
    assert same(one, ref[:1]) and not one[3]["solved_alone"].any()
    d.ctx.set_option("screened_sweep", 1)
    try:
        scr = loop(d, B, k)
        got = batch(d, B, k)
    finally:
        d.ctx.set_option("screened_sweep", 0)
    assert same(got, scr) and not got[3]["solved_alone"].any()
    for s in range(9):                                                    # (certified picks: the exact sweep's supports)
        assert np.array_equal(scr[s][0], ref[s][0]) and scr[s][2] == ref[s][2]
    assert same(batch(d, B, k), ref)


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(cs):
    L = cs._lib
    C = L.C
    A, Ball, k = noisy("256x1024_f32_k20")
    M, N = A.shape
    nsig = 3
    B = np.asfortranarray(Ball[:, :nsig])
    d = cs.Dictionary(A)
    bare = L.Context(0)
    ref = loop(d, B, k)
    fn = L.lib().csmp_ompr_batch

    def message(ctx):
        return L.lib().csmp_last_error(ctx._h).decode()

    def call(ctx, **over):
        a = dict(B=B, dtype=L.F64, ldB=M, nsig=nsig, b_loc=L.HOST, k=k, delta=np.full(1, DELTA), ndelta=1, maxiter=-1, idx=True, val=True, nnz=True)
        a.update(over)
        kk = max(int(a["k"]), 1)
        idx, val = np.full((kk, nsig), 5, np.int64, order="F"), np.full((kk, nsig), 5.0, order="F")
        nnz, it, fl = np.full(nsig, 5, np.int64), np.full(nsig, 5, np.int64), np.full(nsig, 5, np.int32)
        rc = fn(ctx._h, None if a["B"] is None else L.ptr(a["B"]), a["dtype"], L.i64(a["ldB"]), L.i64(a["nsig"]), a["b_loc"], L.i64(a["k"]),
                None if a["delta"] is None else a["delta"].ctypes.data_as(C.POINTER(C.c_double)), L.i64(a["ndelta"]), L.i64(a["maxiter"]),
                L.ptr(idx) if a["idx"] else None, L.ptr(val) if a["val"] else None, L.ptr(nnz) if a["nnz"] else None,
                it.ctypes.data_as(C.POINTER(L.i64)), fl.ctypes.data_as(C.POINTER(C.c_int)))
        untouched = bool(np.all(idx == 5) and np.all(val == 5.0) and np.all(nnz == 5) and np.all(it == 5) and np.all(fl == 5))
        return rc, untouched

    try:
        cases = [("null B", dict(B=None), L.EINVAL), ("null delta", dict(delta=None), L.EINVAL), ("null idx", dict(idx=False), L.EINVAL),
                 ("null val", dict(val=False), L.EINVAL), ("null nnz", dict(nnz=False), L.EINVAL), ("k < 1", dict(k=0), L.EINVAL),
                 ("nsig < 0", dict(nsig=-1), L.EINVAL), ("ndelta 2", dict(delta=np.full(2, DELTA), ndelta=2), L.EINVAL),
                 ("ndelta 0", dict(ndelta=0), L.EINVAL), ("delta nan", dict(delta=np.full(1, np.nan)), L.EINVAL),
                 ("a NaN delta in the last entry", dict(delta=np.array([DELTA, DELTA, np.nan]), ndelta=3), L.EINVAL),
                 ("dtype", dict(dtype=5), L.EINVAL), ("b_loc", dict(b_loc=7), L.EINVAL), ("ldB < M", dict(ldB=M - 1), L.EDIM),
                 ("k > M", dict(k=M + 1), L.ERANGE), ("nsig == 0", dict(nsig=0), L.OK)]
        for name, over, code in cases:
            rc, untouched = call(d.ctx, **over)
            assert rc == code and untouched, (name, rc, untouched)
            if code != L.OK:
                assert "ompr_batch" in message(d.ctx), (name, message(d.ctx))
            assert same(batch(d, B, k), ref), name                         # the context still solves
        rc, untouched = call(d.ctx)                                        # (the harness itself: an accepted call does write)
        assert rc == L.OK and not untouched
        rc, untouched = call(bare)
        assert rc == L.ESTATE and untouched and "ompr_batch" in message(bare)   # no dictionary
    finally:
        d.close()
        bare.close()
    # a failed allocation: CSMP_ENOMEM, and the same context solves afterwards (fail_alloc: the n-th device allocation from now fails;
    # the wide groups' extra slots may fail without failing the call)
    refused = 0
    for n in (1, 2, 30, 90):
        d = cs.Dictionary(A)
        try:
            d.ctx.tune("fail_alloc", n)
            try:
                got = d.ctx.ompr_batch(np.asfortranarray(Ball[:, :5]), k, DELTA)
                assert same(got, loop(d, Ball[:, :5], k)), n
            except cs.CsmpError as e:
                refused += 1
                assert e.code == L.ENOMEM and "ompr_batch" in str(e), (n, e.code, str(e))
            d.ctx.tune("fail_alloc", 0)
            assert same(batch(d, B, k), ref), (n, "after the failed call")
            again = loop(d, B, k)
            assert all(np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) and g[2] == r[2] for g, r in zip(again, ref)), (n, "the single call")
        finally:
            d.close()
    assert refused >= 2
