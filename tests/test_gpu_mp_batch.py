"""GPU tests (pytest -m gpu) of csmp_mp_batch: Matching Pursuit for every column of B on the shared pass of the grouped scheduler.
Every signal keeps csmp_mp's arithmetic -- the pass gives the single sweep's bits per member, k_mp_group picks in k_select's order
and updates with k_mp_update's expression, k_mp_emit restates mp_collect's rule -- so a batch must return the BITS of a caller's
loop over csmp_mp: for every batch size that changes the plan (one group, two groups, wide groups, remainders), on Float32 (even
and odd N) and Float64 dictionaries, under every schedule switch, on the one-at-a-time path, through device pointers, after failed
allocations, and at the benchmark's size."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSIGS = (1, 2, 3, 5, 8, 9, 13, 16, 17, 25)
RTOL = 1e-6  # the suite's tolerance against the oracle


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


def dictionary(M, N, dtype, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(torch.float32 if dtype == np.float32 else torch.float64)
    return At, np.asfortranarray(At.cpu().numpy().T)


def planted(cs, A, ksp, noise, rng):
    xs = cs.sparse_vector(A.shape[1], ksp, rng=rng)
    b = A[:, xs.nzind].astype(np.float64) @ xs.nzval
    return cs.perturb(b, noise, rng=rng) if noise > 0 else b


def signals(cs, A, nsig, seed):
    """noisy planted signals, and among the first five columns: a zero column, a column equal to one atom, a copy of column 0 and a
    noiseless 2-sparse column (MP revisits its two atoms: the merge rule of the output is exercised)"""
    rng = np.random.default_rng(seed)
    cols = [planted(cs, A, 6, 5e-2, rng) for _ in range(nsig)]
    special = [None, np.zeros(A.shape[0]), A[:, A.shape[1] // 3].astype(np.float64), cols[0].copy(), planted(cs, A, 2, 0.0, rng)]
    for j, c in enumerate(special):
        if c is not None and j < nsig:
            cols[j] = c
    return np.asfortranarray(np.stack(cols, axis=1))


def loop(d, B, k):
    """what a caller without the batch form writes: csmp_mp signal by signal, in the batch's output layout"""
    nsig = B.shape[1]
    idx = np.full((k, nsig), -1, np.int64, order="F")
    val = np.zeros((k, nsig), np.float64, order="F")
    nnz = np.zeros(nsig, np.int64)
    for s in range(nsig):
        i, v = d.ctx.mp(B[:, s], k)
        nnz[s] = len(i)
        idx[:len(i), s] = i
        val[:len(i), s] = v
    return idx, val, nnz


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def run(d, B, k, **tunes):
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return d.ctx.mp_batch(B, k)
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


def close(v, ref):
    return np.allclose(v, ref, rtol=RTOL, atol=RTOL * (float(np.max(np.abs(ref))) if len(ref) else 0.0))


@pytest.mark.parametrize("M,N,dtype", [(4096, 6000, np.float32), (4096, 5999, np.float32), (1024, 3000, np.float64)])
def test_bits_of_the_mp_loop(cs, D, M, N, dtype):
    k = 12
    At, A = dictionary(M, N, dtype, 3 + N)
    d = D(At)
    cfg = d.ctx.sweep_config()
    assert cfg["group_max"] == 4 and cfg["group_wide"] == (8 if dtype == np.float32 else 4)
    Ball = signals(cs, A, max(NSIGS), 17 + N)
    ref = loop(d, Ball, k)
    assert ref[2][1] == 0 and ref[2][2] >= 1            # the zero column has no entry (every increment is exactly zero)
    assert np.array_equal(ref[0][:, 3], ref[0][:, 0]) and np.array_equal(ref[1][:, 3], ref[1][:, 0])
    assert ref[2][4] < k                                # the noiseless 2-sparse column revisits atoms
    assert all(ref[2][s] >= 6 for s in range(5, max(NSIGS)))
    for nsig in NSIGS:
        B = np.asfortranarray(Ball[:, :nsig])
        got = d.ctx.mp_batch(B, k)
        want = tuple(np.asfortranarray(x[:, :nsig]) for x in ref[:2]) + (ref[2][:nsig],)
        assert same(got, want), (nsig, got[2], want[2])
        for s in range(nsig):  # the tails
            assert np.all(got[0][got[2][s]:, s] == -1) and np.all(got[1][got[2][s]:, s] == 0.0), (nsig, s)
    # the public function
    xs = cs.mp_batch(d, np.asfortranarray(Ball[:, :9]), k)
    assert len(xs) == 9 and all(np.array_equal(x.nzind, ref[0][:ref[2][s], s]) and np.array_equal(x.nzval, ref[1][:ref[2][s], s]) for s, x in enumerate(xs))


def test_oracle_parity(cs, oracle, D):
    """noisy planted signals, as test_mp_matches_oracle: on noiseless data MP's late picks are decided by rounding noise"""
    nsig = 9
    for (n, m, k, dtype) in [(32, 48, 30, np.float64), (64, 256, 50, np.float32), (37, 101, 25, np.float32)]:
        A, _, _ = cs.sparse_data(n=n, m=m, k=3, rng=n + m, dtype=dtype)
        rng = np.random.default_rng(n * m)
        B = np.asfortranarray(np.stack([planted(cs, A, 3, 5e-2, rng) for _ in range(nsig)], axis=1))
        d = D(A)
        for tunes in ({}, {"pipelines": 3}):  # (dictionaries below 4 MiB keep one stream unless asked)
            idx, val, nnz = run(d, B, k, **tunes)
            for s in range(nsig):
                want = oracle.mp(A, B[:, s], k)
                assert nnz[s] == len(want[0]) and np.array_equal(idx[:nnz[s], s], want[0]), (n, m, s)
                assert close(val[:nnz[s], s], want[1]), (n, m, s)


def test_k_beyond_the_factorisation_bounds(cs, D):
    M, N, k, nsig = 64, 256, 300, 5
    A, _, _ = cs.sparse_data(n=M, m=N, k=4, rng=8, dtype=np.float32)
    rng = np.random.default_rng(2)
    B = np.asfortranarray(np.stack([planted(cs, A, 4, 5e-2, rng) for _ in range(nsig)], axis=1))
    d = D(A)
    ref = loop(d, B, k)
    for tunes in ({}, {"pipelines": 3}, {"pipelines": 2}):
        got = run(d, B, k, **tunes)
        assert same(got, ref), tunes
        assert np.all(got[2] <= min(k, N)) and np.all(got[2] >= 1)


def test_every_schedule_gives_the_same_bits(cs, D):
    M, N, k, nsig = 4096, 7920, 10, 13
    At, A = dictionary(M, N, np.float32, 5)
    d = D(At)
    B = signals(cs, A, nsig, 99)
    ref = loop(d, B, k)
    default = d.ctx.mp_batch(B, k)
    assert same(default, ref)
    schedules = [{"group_wide": 1}, {"group_max": 1}, {"group_max": 2}, {"group_max": 3}, {"pipelines": 1}, {"pipelines": 2},
                 {"pipelines": 3}, {"tick_grid": 203}, {"tick_grid": 17}, {"tick_grid": 7}, {"pipelines": 1, "group_wide": 1}]
    for tunes in schedules:
        assert same(run(d, B, k, **tunes), default), tunes
    for n2 in (2, 5, 8):  # one group: whole on one stream, or its halves on two
        B2 = np.asfortranarray(B[:, :n2])
        want = tuple(np.asfortranarray(x[:, :n2]) for x in ref[:2]) + (ref[2][:n2],)
        for tunes in ({}, {"pipelines": 1}, {"pipelines": 2}, {"pipelines": 3}):
            assert same(run(d, B2, k, **tunes), want), (n2, tunes)
    # the passes were shared: k per group of up to eight signals (13: two groups), every one of them sampled
    d.ctx.profile_enable(True)
    d.ctx.profile_read(reset=True)
    d.ctx.mp_batch(B, k)
    npass, _ = d.ctx.profile_read(reset=True)
    d.ctx.profile_enable(False)
    assert npass == 2 * k, npass
    # CSMP_OPT_PIPELINE 0 and the screened sweep: one signal after the other through csmp_mp's launches
    d.ctx.set_option("pipeline", 0)
    assert same(d.ctx.mp_batch(B, k), ref)
    d.ctx.set_option("pipeline", 1)
    d.ctx.set_option("screened_sweep", 1)  # (csmp_mp's screened steps take the coefficient from the pick's own rescoring: the loop's
    got = d.ctx.mp_batch(B, k)             # bits are those of the loop under the same option)
    ref_screened = loop(d, B, k)
    d.ctx.set_option("screened_sweep", 0)
    assert same(got, ref_screened)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.allclose(got[1], ref[1], rtol=1e-9, atol=1e-12)


def test_dictionary_without_a_shared_pass(cs, D):
    """a column longer than the LDS holds: the sweeps are phased, csmp_sweep_group is 0 and the signals go one after the other"""
    M, N, k, nsig = 32768, 512, 6, 5
    At, A = dictionary(M, N, np.float32, 12)
    d = D(At)
    assert d.ctx.sweep_config()["group_max"] == 0
    B = signals(cs, A, nsig, 4)
    assert same(d.ctx.mp_batch(B, k), loop(d, B, k))


def test_device_form(cs, D):
    import torch
    M, N, k, nsig = 4096, 6000, 9, 11
    At, A = dictionary(M, N, np.float32, 21)
    d = D(At)
    B = signals(cs, A, nsig, 6)
    host = d.ctx.mp_batch(B, k)
    for dt in (torch.float64, torch.float32):
        Bt = torch.from_numpy(np.ascontiguousarray(B.T)).to("cuda").to(dt).contiguous()
        want = host if dt == torch.float64 else d.ctx.mp_batch(np.asfortranarray(B.astype(np.float32)), k)
        idx = torch.full((nsig, k), 7, dtype=torch.int64, device="cuda")
        val = torch.full((nsig, k), 7.0, dtype=torch.float64, device="cuda")
        nnz = torch.full((nsig,), 7, dtype=torch.int64, device="cuda")
        d.ctx.mp_batch_device(Bt, k, idx, val, nnz)
        d.ctx.sync()
        got = (idx.cpu().numpy().T, val.cpu().numpy().T, nnz.cpu().numpy())
        assert same(got, want), dt
        for s in range(nsig):
            assert np.all(got[0][got[2][s]:, s] == -1) and np.all(got[1][got[2][s]:, s] == 0.0)


# ---- arguments: the table tests/test_gpu_batch_args.py runs for the other drivers
AM, AN, ANSIG, AK = 64, 256, 3, 4
OK, EINVAL, ESTATE = 0, -1, -5
_VALID = dict(b_loc=0, out_loc=0, ldB=AM, dtype=1, k=AK, nsig=ANSIG)
_ARG_CASES = [
    ("b_loc", dict(b_loc=7), EINVAL), ("out_loc", dict(out_loc=-1), EINVAL), ("null_B", dict(null_B=True), EINVAL),
    ("ldB_lt_M", dict(ldB=AM - 1), EINVAL), ("dtype", dict(dtype=5), EINVAL), ("k_0", dict(k=0), EINVAL), ("nsig_0", dict(nsig=0), OK),
    ("nsig_neg", dict(nsig=-1), EINVAL), ("no_dictionary", dict(no_dict=True), ESTATE), ("no_dictionary_k_0", dict(no_dict=True, k=0), EINVAL),
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
    idx = np.full((max(k, 1), max(nsig, 1)), 5, np.int64, order="F")
    val = np.full((max(k, 1), max(nsig, 1)), 5.0, np.float64, order="F")
    nnz = np.full(max(nsig, 1), 5, np.int64)
    pB = None if a.get("null_B") else L.ptr(B)
    rc = L.lib().csmp_mp_batch(ctx._h, pB, a["dtype"], L.i64(a["ldB"]), L.i64(nsig), a["b_loc"], L.i64(k), L.ptr(idx), L.ptr(val),
                               L.ptr(nnz), a["out_loc"])
    return rc, idx, val, nnz


@pytest.mark.parametrize("over,want", [pytest.param(o, w, id=name) for name, o, w in _ARG_CASES])
def test_arguments(cs, contexts, over, want):
    L = cs._lib
    with_dict, bare = contexts
    ctx = bare if over.get("no_dict") else with_dict
    rc, idx, val, nnz = _call(L, ctx, dict(_VALID, **over))
    assert rc == want
    if rc != OK or over.get("nsig") == 0:  # nothing was touched
        assert np.all(idx == 5) and np.all(val == 5.0) and np.all(nnz == 5)
    if ctx is with_dict:  # the context is still good for a valid call
        rc, idx, val, nnz = _call(L, ctx, _VALID)
        assert rc == OK and np.all(nnz >= 1) and np.all(nnz <= AK)


def test_create_batch_destroy_cycles_hold_nothing(cs):
    L = cs._lib
    A, _, _ = cs.sparse_data(n=96, m=384, k=6, rng=11, dtype=np.float32)
    rng = np.random.default_rng(1)
    B = np.asfortranarray(np.stack([planted(cs, A, 6, 5e-2, rng) for _ in range(11)], axis=1))
    gc.collect()
    base = L.live_resources()
    want = None
    for c in range(50):
        d = cs.Dictionary(A)
        d.ctx.tune("pipelines", (3, 2, 1, 0)[c % 4])  # (two streams for this small dictionary too: the twin context and its stream)
        got = d.ctx.mp_batch(B, 8)
        want = got if want is None else want
        assert same(got, want), c
        d.close()
    gc.collect()
    live = L.live_resources()
    assert live == base, (live, base)
    assert all(live[key] - base[key] == 0 for key in live)


def test_every_allocation_may_fail(cs):
    """fail_alloc = n makes the n-th device allocation from now fail for real (the hook tests/test_gpu_leaks.py uses).  For every n
    until the call goes through twice in a row: a failing call returns a status, and the same context then returns the clean
    context's bits.  The allocations of the wide groups' slots come last, and a failure among them is not a failure of the call: the
    batch runs groups of four on the slots it has -- the same bits."""
    L = cs._lib
    A, _, _ = cs.sparse_data(n=256, m=1024, k=6, rng=21, dtype=np.float32)
    rng = np.random.default_rng(7)
    nsig, k = 9, 6
    B = np.asfortranarray(np.stack([planted(cs, A, 6, 5e-2, rng) for _ in range(nsig)], axis=1))
    gc.collect()
    base = L.live_resources()
    clean = cs.Dictionary(A)
    clean.ctx.tune("pipelines", 3)
    assert clean.ctx.sweep_config()["group_wide"] == 8
    want = clean.ctx.mp_batch(B, k)
    assert same(want, loop(clean, B, k))
    clean.close()
    n, seen_ok, failed = 0, 0, 0
    while seen_ok < 2 and n < 2000:
        n += 1
        d = cs.Dictionary(A)
        d.ctx.tune("pipelines", 3)
        d.ctx.tune("fail_alloc", n)
        try:
            got = d.ctx.mp_batch(B, k)
            assert same(got, want), (n, "the call went through with a result of its own")
            seen_ok += 1
        except cs.CsmpError as e:
            seen_ok = 0
            failed += 1
            assert e.code in (L.EHIP, L.ENOMEM), (n, e.code, str(e))
        d.ctx.tune("fail_alloc", 0)
        assert same(d.ctx.mp_batch(B, k), want), (n, "after the failed call")
        d.close()
    assert n < 2000 and failed >= 3 * 30, (n, failed)  # (the call's staging and the context's three further narrow slots at the least)
    gc.collect()
    assert L.live_resources() == base


def test_full_size(cs, oracle, D):
    """the benchmark's dictionary: 4096 x 65536 Float32, sixteen signals, 64 steps -- the loop's bits for all sixteen, the oracle's
    support and coefficients for three"""
    M, N, k, nsig = 4096, 65536, 64, 16
    At, A = dictionary(M, N, np.float32, 2024)
    d = D(At)
    rng = np.random.default_rng(5)
    B = np.asfortranarray(np.stack([planted(cs, A, 16, 5e-2, rng) for _ in range(nsig)], axis=1))
    got = d.ctx.mp_batch(B, k)
    assert same(got, loop(d, B, k))
    idx, val, nnz = got
    for s in (0, 7, 15):
        want = oracle.mp(A, B[:, s], k)
        assert nnz[s] == len(want[0]) and np.array_equal(idx[:nnz[s], s], want[0]), s
        assert close(val[:nnz[s], s], want[1]), s
