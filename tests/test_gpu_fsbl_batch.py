"""GPU tests (pytest -m gpu) of csmp_fsbl_batch / csmp_rmps_batch: fsbl / rmps for every column of B, the members of a group in lockstep
on shared launches.  Every member keeps csmp_fsbl's arithmetic -- the shared pass gives the single sweep's bits per member, the group
kernels call the single kernels' bodies on the member's own buffers, a member starts as csmp_fsbl does -- so a batch must return the
BITS of a caller's loop over csmp_fsbl / csmp_rmps: X, alpha, iterations, converged and the histories, whatever the batch size, the
group sizes, the order the slots are refilled in, the noise variances and the warm starts."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsbl_twin as tw  # noqa: E402
from test_gpu_bp_batch import signals as plain_signals, torch_dictionary  # noqa: E402

pytestmark = pytest.mark.gpu

NSIGS = (1, 2, 3, 5, 8, 9, 13)
CASES = ("32x48k8s19_f64", "100x257k20s23_f32", "130x300k25s7_f32", "257x300_f32", "48x32_f64")
DELETING = CASES[:3]          # the cases whose own y (column 4) meets deletions
S2 = tw.SIGMA ** 2
SOLVERS = ("fsbl", "rmps")
_problems = {}


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


def problem(name):
    """(A, B): the case's dictionary and 13 signals -- column s has 1 + (3 s) % max(2, M // 4) planted atoms with values N(0, 1) + sign
    plus noise of norm sigma / 2, column 1 is zero, column 4 is the case's own y; made once per case, never changed"""
    if name not in _problems:
        A, _, _, y = tw.case_data(name)
        M, N = A.shape
        A64 = np.asarray(A, np.float64)
        rng = np.random.default_rng(M * N + 1)
        cols = []
        for s in range(max(NSIGS)):
            k = 1 + (3 * s) % max(2, M // 4)
            sup = rng.choice(N, k, replace=False)
            val = rng.standard_normal(k) + np.sign(rng.standard_normal(k))
            e = rng.standard_normal(M)
            cols.append(A64[:, sup] @ val + e * (tw.SIGMA / 2 / np.linalg.norm(e)))
        cols[1] = np.zeros(M)
        cols[4] = np.asarray(y, np.float64).copy()
        _problems[name] = (A, np.asfortranarray(np.stack(cols, axis=1)))
    return _problems[name]


def flat(res):
    X, info = res
    return X, info["alpha"], np.asarray(info["iterations"]), np.asarray(info["converged"]), [list(h) for h in info["history"]]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def cut(ref, n):
    return (np.asfortranarray(ref[0][:, :n]), np.asfortranarray(ref[1][:, :n]), ref[2][:n], ref[3][:n], ref[4][:n])


def loop(d, solver, B, sigma2=S2, alpha=None, **kw):
    """what a caller without the batch form writes: csmp_fsbl / csmp_rmps column by column on the same Dictionary"""
    N, nsig = d.shape[1], B.shape[1]
    s2 = np.broadcast_to(np.asarray(sigma2, np.float64), (nsig,))
    X = np.zeros((N, nsig), np.float64, order="F")
    Al = np.zeros((N, nsig), np.float64, order="F")
    its, conv, hist = np.zeros(nsig, np.int64), np.zeros(nsig, bool), []
    for s in range(nsig):
        a = None if alpha is None else np.ascontiguousarray(alpha[:, s])
        X[:, s], info = getattr(d.ctx, solver)(np.ascontiguousarray(B[:, s]), float(s2[s]), alpha=a, **kw)
        Al[:, s], its[s], conv[s] = info["alpha"], info["iterations"], info["converged"]
        hist.append(list(info["history"]))
    return X, Al, its, conv, hist


def batch(d, solver, B, sigma2=S2, alpha=None, tunes=None, **kw):
    tunes = tunes or {}
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return flat(getattr(d.ctx, solver + "_batch")(B, sigma2, alpha=alpha, **kw))
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


# ------------------------------------------------------------------------------------------ 1. bits of the loop
@pytest.mark.parametrize("name", CASES)
def test_bits_of_the_loop(cs, D, name):
    A, Ball = problem(name)
    N = A.shape[1]
    d = D(A)
    for solver in SOLVERS:
        ref = loop(d, solver, Ball)
        dels = [sum(1 for a, _ in h if a == tw.ACT_DEL) for h in ref[4]]
        print(f"{name} {solver}: iterations {ref[2].tolist()}, converged {ref[3].astype(int).tolist()}, deletions {dels}")
        # the preconditions, on the loop's own output: a trivial input cannot pass
        assert len(set(ref[2].tolist())) >= 3
        if name in DELETING:
            assert sum(dels) >= 1
        assert np.all(ref[3])
        assert np.all(ref[0][:, 1] == 0.0) and ref[2][1] == (1 if solver == "fsbl" else 0) and ref[4][1] == []   # the zero column
        for nsig in NSIGS:
            got = batch(d, solver, np.asfortranarray(Ball[:, :nsig]))
            assert same(got, cut(ref, nsig)), (solver, nsig, got[2], ref[2][:nsig])
        assert same(batch(d, solver, Ball), ref)                              # two runs: the same bits
        for kw in (dict(maxiter=1), dict(maxiter=5)) + ((dict(maxiter=2, maxiter_acquisition=3),) if solver == "rmps" else ()):
            capped = loop(d, solver, Ball, **kw)
            if solver == "fsbl" or "maxiter_acquisition" in kw:
                assert not np.all(capped[3]), kw                                  # caps reached, not converged
            for nsig in (2, 9, 13):
                assert same(batch(d, solver, np.asfortranarray(Ball[:, :nsig]), **kw), cut(capped, nsig)), (solver, kw, nsig)
    # the public functions, against the public fsbl / rmps
    for fb, f1 in ((cs.fsbl_batch, cs.fsbl), (cs.rmps_batch, cs.rmps)):
        xs, info = fb(d, Ball[:, :9], S2, return_info=True)
        assert len(xs) == 9 and len(fb(d, Ball[:, :9], S2)) == 9
        for s, x in enumerate(xs):
            one, oi = f1(d, Ball[:, s], S2, return_info=True)
            assert x.n == N and np.array_equal(x.to_dense(), one), s
            assert info["iterations"][s] == oi["iterations"] and info["converged"][s] == oi["converged"] and info["history"][s] == oi["history"]
            assert np.array_equal(info["alpha"][:, s], oi["alpha"])


# ------------------------------------------------------------------------------------------ 2. a noise variance per signal
@pytest.mark.parametrize("solver", SOLVERS)
def test_sigma2_per_signal(cs, D, solver):
    A, Ball = problem(CASES[1])
    nsig = 9
    B = np.asfortranarray(Ball[:, :nsig])
    d = D(A)
    s2 = np.array([S2, 4e-4, S2, 2.5e-5, 1e-3, S2, 9e-4, 1e-5, 2e-4])              # with a repeat
    ref = loop(d, solver, B, s2)
    assert same(batch(d, solver, B, s2), ref)
    scalar = batch(d, solver, B, S2)
    assert same(scalar, loop(d, solver, B, S2)) and not same(scalar, ref)       # (the variances do reach the columns)
    assert np.array_equal(scalar[0][:, 0], ref[0][:, 0])                        # ... and an equal variance gives equal bits


# ------------------------------------------------------------------------------------------ 3. warm starts
@pytest.mark.parametrize("solver", SOLVERS)
def test_warm_starts(cs, D, solver):
    import torch
    A, Ball = problem(CASES[2])
    N = A.shape[1]
    nsig = 9
    B = np.asfortranarray(Ball[:, :nsig])
    d = D(A)
    alpha = np.full((N, nsig), np.inf, order="F")
    for s in range(nsig):                                                       # fsbl(maxiter = 0 (cold), 3, 12) of each signal, in turn
        t = (0, 3, 12)[s % 3]
        if t:
            alpha[:, s] = d.ctx.fsbl(np.ascontiguousarray(B[:, s]), S2, maxiter=t)[1]["alpha"]
    counts = np.isfinite(alpha).sum(axis=0)
    print(f"active atoms of the warm starts: {counts.tolist()}")
    assert len(set(counts.tolist())) >= 3 and counts[0] == 0
    ref = loop(d, solver, B, alpha=alpha)
    assert same(batch(d, solver, B, alpha=alpha), ref)
    assert not same(ref, loop(d, solver, B))
    short = dict(maxiter=4) if solver == "fsbl" else dict(maxiter=1, maxiter_acquisition=2, maxiter_deletion=2)
    first = loop(d, solver, B, **short)
    second = loop(d, solver, B, alpha=first[1], **short)
    assert not np.array_equal(first[1], second[1])
    # alpha_out aliasing alpha_in on the device: two calls in place against two looped calls
    Bt = torch.from_numpy(np.ascontiguousarray(B.T)).cuda().T
    Xt = torch.zeros((nsig, N), dtype=torch.float64, device="cuda").T
    At = torch.full((nsig, N), float("inf"), dtype=torch.float64, device="cuda").T
    run = getattr(d.ctx, solver + "_batch_device")
    i1 = run(Bt, S2, Xt, None, At, history_cap=64, **short)
    assert np.array_equal(Xt.cpu().numpy(), first[0]) and np.array_equal(At.cpu().numpy(), first[1]) and i1["history"] == first[4]
    i2 = run(Bt, S2, Xt, At, At, history_cap=64, **short)
    assert np.array_equal(Xt.cpu().numpy(), second[0]) and np.array_equal(At.cpu().numpy(), second[1]) and i2["history"] == second[4]
    assert np.array_equal(i2["iterations"], second[2]) and np.array_equal(i2["converged"], second[3])
    # continuing a batch from its own alpha equals the loop doing the same
    h1 = batch(d, solver, B, **short)
    assert same(h1, first) and same(batch(d, solver, B, alpha=h1[1], **short), second)


# ------------------------------------------------------------------------------------------ 4. history caps
@pytest.mark.parametrize("solver", SOLVERS)
def test_history_caps(cs, D, solver):
    A, Ball = problem(CASES[0])
    B = np.asfortranarray(Ball[:, :9])
    d = D(A)
    full = batch(d, solver, B)
    assert max(len(h) for h in full[4]) > 7
    for cap in (0, 7):
        part = batch(d, solver, B, history_cap=cap)
        assert same(part[:4] + (full[4],), full) and part[4] == [h[:cap] for h in full[4]], cap


# ------------------------------------------------------------------------------------------ 5. every pass instantiation
@pytest.mark.parametrize("scalar_loads", [0, 1], ids=["vector_loads", "scalar_loads"])
@pytest.mark.parametrize("M,N,dtype,group,wide", [(4096, 4200, np.float32, 4, 8), (3000, 3100, np.float32, 4, 8), (1024, 1500, np.float64, 4, 4),
                                                  (256, 4096, np.float32, 4, 8)],
                         ids=["whole_units_wide", "clamped_loads", "f64_four_waves", "short_columns"])
def test_every_pass_instantiation(cs, D, M, N, dtype, group, wide, scalar_loads):
    At, A = torch_dictionary(M, N, dtype, 7 + N)
    d = D(At)
    cfg = d.ctx.sweep_config()
    print(f"{M} x {N}: group_max {cfg['group_max']}, group_wide {cfg['group_wide']}")
    assert cfg["group_max"] == group and cfg["group_wide"] == wide          # (a shared pass: the batch is not its own loop)
    B = plain_signals(A, 9)
    d.ctx.tune("fsbl_scalar", scalar_loads)
    try:
        for solver, kw in (("fsbl", dict(maxiter=3)), ("rmps", dict(maxiter=3, maxiter_acquisition=3, maxiter_deletion=3))):
            ref = loop(d, solver, B, **kw)
            steps = [len(h) for h in ref[4]]
            assert steps[1] == 0 and min(steps[:1] + steps[2:]) >= 1                # every signal but the zero column steps
            assert same(batch(d, solver, B, **kw), ref), solver
    finally:
        d.ctx.tune("fsbl_scalar", 0)


# ------------------------------------------------------------------------------------------ 6. schedule switches
@pytest.mark.parametrize("solver", SOLVERS)
def test_schedule_switches(cs, D, solver):
    A, Ball = problem(CASES[2])
    B = np.asfortranarray(Ball[:, :9])
    d = D(A)
    ref = loop(d, solver, B)
    assert same(batch(d, solver, B), ref)
    for tunes in ({"group_max": 1}, {"group_max": 2}, {"group_max": 3}, {"group_max": 4}, {"group_wide": 1}):
        assert same(batch(d, solver, B, tunes=tunes), ref), tunes
    d.ctx.tune("sweep_dyn", 1)  # no shared pass: the batch takes the loop
    try:
        assert d.ctx.sweep_config()["group_max"] == 0
        assert same(batch(d, solver, B), loop(d, solver, B))
    finally:
        d.ctx.tune("sweep_dyn", 0)
    d.ctx.set_option("screened_sweep", 1)  # the screened sweeps: signal by signal, the loop's bits under the same option
    try:
        assert same(batch(d, solver, B), loop(d, solver, B))
    finally:
        d.ctx.set_option("screened_sweep", 0)
    assert same(batch(d, solver, B), ref)


# ------------------------------------------------------------------------------------------ 7. device pointers
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["B_f32", "B_f64"])
def test_device_pointers(cs, D, dtype):
    import torch
    A, Ball = problem(CASES[1])
    M, N = A.shape
    nsig, ldB, ldX, ldA = 9, M + 3, N + 5, N + 2
    Bh = np.asfortranarray(Ball[:, :nsig].astype(dtype))
    d = D(A)
    warm = np.full((N, nsig), np.inf, order="F")
    warm[:, 2] = d.ctx.fsbl(np.ascontiguousarray(Bh[:, 2]), S2, maxiter=5)[1]["alpha"]
    for solver in SOLVERS:
        want = batch(d, solver, Bh, alpha=warm)
        assert same(want, loop(d, solver, Bh, alpha=warm))
        buf = torch.full((nsig, ldB), 3.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
        buf[:, :M] = torch.from_numpy(np.ascontiguousarray(Bh.T)).cuda()
        xbuf = torch.full((nsig, ldX), 7.0, dtype=torch.float64, device="cuda")
        abuf = torch.full((nsig, ldA), 9.0, dtype=torch.float64, device="cuda")
        obuf = torch.full((nsig, ldA), 11.0, dtype=torch.float64, device="cuda")
        abuf[:, :N] = torch.from_numpy(np.ascontiguousarray(warm.T)).cuda()
        Bt, Xt, Ait, Aot = buf.T[:M], xbuf.T[:N], abuf.T[:N], obuf.T[:N]
        assert Bt.stride() == (1, ldB) and Xt.stride() == (1, ldX) and Ait.stride() == (1, ldA)
        for _ in range(2):                                       # two runs: the same bits
            info = getattr(d.ctx, solver + "_batch_device")(Bt, S2, Xt, Ait, Aot, history_cap=4 * N)
            got = (Xt.cpu().numpy(), Aot.cpu().numpy(), info["iterations"], info["converged"], info["history"])
            assert same(got, want), solver
        assert np.all(xbuf[:, N:].cpu().numpy() == 7.0) and np.all(obuf[:, N:].cpu().numpy() == 11.0)   # the padding is untouched
        assert np.all(buf[:, M:].cpu().numpy() == 3.0) and np.array_equal(buf[:, :M].cpu().numpy().T, Bh)   # B is read only
        assert np.array_equal(abuf[:, :N].cpu().numpy().T, warm) and np.all(abuf[:, N:].cpu().numpy() == 9.0)   # alpha_in too


# ------------------------------------------------------------------------------------------ 8. the other solvers
def test_other_solvers_are_undisturbed(cs, D):
    A, Ball = problem(CASES[1])
    B = np.asfortranarray(Ball[:, :5])
    d = D(A)
    b0 = np.ascontiguousarray(B[:, 0])

    def others(ctx):
        xf, fi = ctx.fsbl(b0, S2)
        xr, ri = ctx.rmps(b0, S2)
        xb, ib = ctx.bp(b0, maxiter=64)
        xd, idn = ctx.bpd(b0, 0.05, maxiter=64)
        xi, rni = ctx.ista(b0, 0.05, maxiter=20, stepsize=0.1)
        return ((xf, fi["alpha"], np.array(fi["history"]), xr, ri["alpha"], np.array(ri["history"]), xb, np.float64(ib["resnorm"]), xd,
                 np.float64(idn["resnorm"]), xi, np.float64(rni)), (ib["factored"], idn["factored"]))

    before, fac = others(d.ctx)
    assert fac == (True, True)
    steps = d.ctx.bench_fsbl(1)                                   # csmp_fsbl's own kept state is there ...
    for solver in SOLVERS:
        got = batch(d, solver, B)
        assert same(got, loop(d, solver, B))
    after, fac = others(d.ctx)
    assert fac == (False, False)                                  # bp's and bpd's kept factors were neither dropped nor rebuilt
    assert all(np.array_equal(x, y) for x, y in zip(after, before))
    assert set(d.ctx.bench_fsbl(1)) == set(steps)                 # ... and still is
    for solver in SOLVERS:
        assert same(batch(d, solver, B), loop(d, solver, B))


# ------------------------------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("solver", SOLVERS)
def test_refusals(cs, solver):
    L = cs._lib
    C = L.C
    A, Ball = problem(CASES[0])
    M, N = A.shape
    nsig = 3
    B = np.asfortranarray(Ball[:, :nsig])
    d = cs.Dictionary(A)
    bare = L.Context(0)
    want = batch(d, solver, B)
    fn = getattr(L.lib(), f"csmp_{solver}_batch")
    ncaps = 1 if solver == "fsbl" else 3

    def call(ctx, **over):
        Nc = over.get("N", N)
        a = dict(B=B, dtype=L.F64, ldB=M, nsig=nsig, b_loc=L.HOST, sigma2=np.full(1, S2), nsigma2=1, caps=(8,) * ncaps, min_increase=1e-6,
                 alpha_in=None, ld_in=Nc, ldX=Nc, alpha_out=True, ld_out=Nc, x_loc=L.HOST, cap=4, X=True)
        a.update(over)
        a.pop("N", None)
        X = np.full((Nc, nsig), 5.0, order="F")                  # (Nc: another dictionary's columns, the tall one's below)
        Ao = np.full((Nc, nsig), 5.0, order="F")
        hist = np.full((nsig, 4, 2), 5, np.int64)
        it, fl = np.full(nsig, 5, np.int64), np.full(nsig, 5, np.int32)
        rc = fn(ctx._h, None if a["B"] is None else L.ptr(a["B"]), a["dtype"], L.i64(a["ldB"]), L.i64(a["nsig"]), a["b_loc"],
                None if a["sigma2"] is None else L.ptr(a["sigma2"]), L.i64(a["nsigma2"]), *[L.i64(c) for c in a["caps"]], C.c_double(a["min_increase"]),
                None if a["alpha_in"] is None else L.ptr(a["alpha_in"]), L.i64(a["ld_in"]), L.ptr(X) if a["X"] else None, L.i64(a["ldX"]),
                L.ptr(Ao) if a["alpha_out"] else None, L.i64(a["ld_out"]), a["x_loc"], L.ptr(hist), L.i64(a["cap"]),
                it.ctypes.data_as(C.POINTER(L.i64)), fl.ctypes.data_as(C.POINTER(C.c_int)))
        return rc, bool(np.all(X == 5.0) and np.all(Ao == 5.0) and np.all(hist == 5) and np.all(it == 5) and np.all(fl == 5))

    def warm(v):
        a = np.full((N, nsig), np.inf, order="F")
        a[N - 1, nsig - 1] = v                                   # (in the last column: every signal is checked before any runs)
        return a

    try:
        cases = [("ldB < M", dict(ldB=M - 1), L.EDIM), ("ldX < N", dict(ldX=N - 1), L.EDIM), ("ld_alpha_in < N", dict(alpha_in=warm(1.0), ld_in=N - 1), L.EDIM),
                 ("ld_alpha_out < N", dict(ld_out=N - 1), L.EDIM), ("nsig < 0", dict(nsig=-1), L.EINVAL), ("nsig == 0", dict(nsig=0), L.OK),
                 ("nsigma2 2", dict(sigma2=np.full(2, S2), nsigma2=2), L.EINVAL), ("nsigma2 0", dict(nsigma2=0), L.EINVAL),
                 ("sigma2 0", dict(sigma2=np.zeros(1)), L.EINVAL), ("sigma2 < 0", dict(sigma2=np.full(1, -S2)), L.EINVAL),
                 ("sigma2 nan", dict(sigma2=np.full(1, np.nan)), L.EINVAL), ("sigma2 inf", dict(sigma2=np.full(1, np.inf)), L.EINVAL),
                 ("a bad sigma2 in the last entry", dict(sigma2=np.array([S2, S2, 0.0]), nsigma2=3), L.EINVAL),
                 ("null sigma2", dict(sigma2=None), L.EINVAL), ("null B", dict(B=None), L.EINVAL), ("null X", dict(X=False), L.EINVAL),
                 ("dtype", dict(dtype=5), L.EINVAL), ("b_loc", dict(b_loc=7), L.EINVAL), ("x_loc", dict(x_loc=-1), L.EINVAL),
                 ("min_increase < 0", dict(min_increase=-1e-6), L.EINVAL), ("min_increase nan", dict(min_increase=float("nan")), L.EINVAL),
                 ("history_cap < 0", dict(cap=-1), L.EINVAL),
                 ("alpha 0", dict(alpha_in=warm(0.0)), L.EINVAL), ("alpha < 0", dict(alpha_in=warm(-1.0)), L.EINVAL),
                 ("alpha nan", dict(alpha_in=warm(np.nan)), L.EINVAL)]
        for q in range(ncaps):
            caps = [8] * ncaps
            caps[q] = 0
            cases.append((f"cap {q} < 1", dict(caps=tuple(caps)), L.EINVAL))
        for name, over, code in cases:
            rc, untouched = call(d.ctx, **over)
            assert rc == code and untouched, (name, rc, untouched)
            assert same(batch(d, solver, B), want), name          # the context still solves
        rc, untouched = call(d.ctx, alpha_in=warm(2.0))          # (the harness itself: an accepted call does write)
        assert rc == L.OK and not untouched
        rc, untouched = call(bare)
        assert rc == L.ESTATE and untouched                      # no dictionary
        # more than 2^19 rows: CSMP_ERANGE before anything is allocated or written (fsbl asks for no M <= N: two columns do, 4 MiB)
        Mt, Nt = 2 ** 19 + 1, 2
        tall = np.asfortranarray(np.random.default_rng(3).standard_normal((Mt, Nt)).astype(np.float32))
        d.ctx.set_dictionary(tall)
        Bt = np.zeros((Mt, nsig), order="F")
        Bt[:, 0] = tall[:, 1]
        rc, untouched = call(d.ctx, B=Bt, ldB=Mt, N=Nt)
        assert rc == L.ERANGE and untouched, (rc, untouched)
        rc, untouched = call(d.ctx, B=Bt, ldB=Mt, N=Nt, nsig=1)  # (the lone signal's path refuses alike)
        assert rc == L.ERANGE and untouched, (rc, untouched)
        with pytest.raises(cs.CsmpError) as e:
            getattr(d.ctx, solver)(Bt[:, 0].copy(), S2)          # as the single call does
        assert e.value.code == L.ERANGE
        d.ctx.set_dictionary(A)
        assert same(flat(getattr(d.ctx, solver + "_batch")(B, S2)), want)   # the context still solves
    finally:
        d.close()
        bare.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        with pytest.raises(cs.CsmpError) as e:
            getattr(S.ctx, solver + "_batch")(B, S2)
        assert e.value.code == L.ESTATE
    finally:
        S.close()


# ------------------------------------------------------------------------------------------ 10. allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_bp_batch.py's pattern: every device allocation of a fsbl_batch call fails in turn with CSMP_ENOMEM, the same context
    then returns the clean context's bits, and the library holds what it held before.  Least failures: the staged B, FsblBatchBuf's 11
    (C^-1, the M-vectors, alpha, S, Q, w, x, the two partials, the records, the norms) and one or more for each of the four solver slots
    of a group -- 16.  (A Float64 dictionary: no wide groups, whose slots may fail without failing the call.)"""
    L = cs._lib
    A, Ball = problem(CASES[0])
    B = np.asfortranarray(Ball[:, :5])
    gc.collect()
    base = L.live_resources()
    clean = cs.Dictionary(A)
    assert clean.ctx.sweep_config()["group_wide"] == clean.ctx.sweep_config()["group_max"] == 4
    want = batch(clean, "fsbl", B)
    assert same(want, loop(clean, "fsbl", B))
    clean.close()
    n, seen_ok, failed = 0, 0, 0
    while seen_ok < 2 and n < 600:
        n += 1
        d = cs.Dictionary(A)
        d.ctx.tune("fail_alloc", n)
        try:
            got = batch_raw(d, B)
            assert same(got, want), n
            seen_ok += 1
        except cs.CsmpError as e:
            seen_ok = 0
            failed += 1
            assert e.code == L.ENOMEM, (n, e.code, str(e))
            assert "R x size(A,1)^2 doubles" in str(e), str(e)      # the message names the size
        d.ctx.tune("fail_alloc", 0)
        assert same(batch_raw(d, B), want), (n, "after the failed call")
        d.close()
    print(f"fsbl_batch: {failed} allocations failed in turn")
    assert n < 600 and failed >= 16
    gc.collect()
    assert L.live_resources() == base


def batch_raw(d, B):
    return flat(d.ctx.fsbl_batch(B, S2))


# ------------------------------------------------------------------------------------------ 11. twin parity
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", DELETING)
def test_parity_with_the_twin(cs, D, name, solver):
    A, Ball = problem(name)
    xt, it = tw.case_twin(name, solver)
    d = D(A)
    X, Al, its, conv, hist = batch(d, solver, Ball)
    x, al = X[:, 4], Al[:, 4]
    fin = np.isfinite(it["alpha"])
    assert np.array_equal(np.isfinite(al), fin) and np.array_equal(x != 0, fin)
    ex = float(np.max(np.abs(x - xt)) / np.max(np.abs(xt)))
    ea = float(np.max(np.abs(al[fin] - it["alpha"][fin]) / it["alpha"][fin]))
    print(f"{name} {solver}: {len(hist[4])} steps (twin {len(it['history'])}), max|x - twin| / max|x| = {ex:.3e}, max rel |alpha - twin| = {ea:.3e}")
    assert hist[4] == [tuple(h) for h in it["history"]] and any(a == tw.ACT_DEL for a, _ in hist[4])
    assert its[4] == it["iterations"] and conv[4] == it["converged"]
    assert ex <= tw.RTOL and ea <= tw.RTOL
