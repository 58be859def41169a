"""GPU tests (pytest -m gpu) of every product-sweep instantiation the host dispatch can launch, at shapes of a few megabytes.

tests/sweep_plan.py is a Python twin of that dispatch; every case here asserts sweep_config() against the twin before it launches,
and tests/test_sweep_plan_static.py checks that the case tables below (CASES_*: read there through reached()) reach every sweep-family
kernel of the code object, or that the kernel stands in its UNREACHED table with the reason.

Reference: A.astype(longdouble).T @ r on the exactly promoted values; "exact" is int64 arithmetic on integer data (entries in
[-8, 8], r in [-16, 16]: every partial sum is an integer below 2^53, so Float64 makes no rounding error in ANY order).
Bound: a lane's sum is one fma chain over its rows followed by the six additions of the butterfly, so
|c_j - ref_j| <= gamma_n sum_i |a_ij r_i|, n = chain_length() of the twin (rows of the image per lane + 6; short: NCH * VEC + 6;
phases: + one addition per further stage), u = 2^-53.  No tolerance is tuned."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_plan as sp  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MIB8 = 8 << 20


def close(v, ref, tol=1e-9):  # (the FR tests' tolerance, tests/test_gpu_shapes.py)
    return np.allclose(v, ref, rtol=tol, atol=tol * (float(np.max(np.abs(ref))) if len(ref) else 0.0))


@pytest.fixture
def D(cs):
    """dictionaries of ONE test, closed when it ends"""
    made = []

    def make(A, **tunes):
        d = cs.Dictionary(A)
        made.append(d)
        for key, v in tunes.items():
            d.ctx.tune(key, v)
        return d
    yield make
    for d in made:
        d.close()


@pytest.fixture(scope="module")
def cus(cs):
    d = cs.Dictionary(np.asfortranarray(np.eye(4, dtype=F32)))
    n = d.ctx.device_info()[1]
    d.close()
    return n


def int_dict(M, N, dtype, seed):
    g = np.random.default_rng(seed)
    return np.asfortranarray(g.integers(-8, 9, size=(M, N)).astype(dtype))


def int_vec(M, seed):
    return np.random.default_rng(seed).integers(-16, 17, size=M).astype(F64)


def gauss_dict(M, N, dtype, seed):
    g = np.random.default_rng(seed)
    A = g.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    return np.asfortranarray(A.astype(dtype))


def exact(A, r):
    return A.astype(np.int64).T @ r.astype(np.int64)


def bound(A, r, n):
    u = np.longdouble(2.0) ** -53
    gamma = n * u / (1 - n * u)
    return np.asarray(gamma * (np.abs(A).astype(np.longdouble).T @ np.abs(r).astype(np.longdouble)), dtype=np.longdouble)


def ncols(M, dtype, N):
    """N, or the most columns an 8-MiB dictionary of M rows holds"""
    return max(1, min(N, MIB8 // (M * np.dtype(dtype).itemsize)))


def check_config(d, p):
    cfg = d.ctx.sweep_config()
    want = p.config()
    assert cfg == want, (cfg, want)


def check_sweep_exact(d, A, r, topk=7):
    N = A.shape[1]
    ref = np.abs(exact(A, r)).astype(F64)
    k = min(topk, N, A.shape[0])  # (csmp_sweep takes no topk above size(A,1), host/gomp_sp.hpp)
    got, ti, tv = d.ctx.sweep(r, topk=k)
    assert np.array_equal(got, ref), (np.flatnonzero(got != ref)[:8], got[got != ref][:8], ref[got != ref][:8])
    order = np.lexsort((np.arange(N), -ref))[:k]  # descending |c|, ties to the lower index
    assert np.array_equal(ti, order), (ti, order)
    assert np.array_equal(tv, ref[order])
    # topk = 1 is the sweep's FUSED arg-max (the partials of the body itself, host/gomp_sp.hpp csmp_sweep); topk > 1 selects from c
    _, t1, v1 = d.ctx.sweep(r, topk=1, want_abs=False)
    assert t1[0] == order[0] and v1[0] == ref[order[0]], (t1[0], order[0])


def plant_ties(A, r, cols):
    """the columns `cols` become +-8 sign(r): |c| = 8 sum|r|, the largest value any column can reach -- they tie at the top"""
    s = np.where(r >= 0, 8.0, -8.0)
    for n, c in enumerate(sorted(set(int(c) for c in cols if 0 <= c < A.shape[1]))):
        A[:, c] = (s if n % 2 == 0 else -s).astype(A.dtype)


def tie_columns(p, kernel, N, nblk):
    """columns that tie across waves, across workgroups, within a wave's sequence and across its 64-column store, by the twin's map"""
    body = sp.body_of(kernel)
    if body == "dyn":  # (claimed at run time: no static map)
        return [0, 1, N // 2, N - 1]
    nch = p.short_nch if body == "short" else 0
    w0 = sp.wave_columns(body, 0, 0, N, nblk, nch)
    w1 = sp.wave_columns(body, 0, 1, N, nblk, nch)
    wl = sp.wave_columns(body, nblk - 1, 0, N, nblk, nch)
    st = 64 if body != "short" else 384
    picks = [w0[0] if w0 else 0, N - 1]
    if len(w0) > 1:
        picks.append(w0[1])  # (short: a neighbouring lane row of the same unit; else the wave's next column)
    if len(w0) > st:
        picks += [w0[st - 1], w0[st]]
    if w1:
        picks.append(w1[0])
    if wl:
        picks.append(wl[0])
    return picks[:7]


# ------------------------------------------------------------------------------------------ (a) exact integer sweeps
def _rows(dtype):
    return 256 if dtype == F32 else 128


def _gen_cases():
    out = []
    for dtype in (F32, F64):
        rows = _rows(dtype)
        for U in (4, 8, 16):
            # fewer chunks than a unit (down to M = 5 and 32), one unit, the ring (32 chunks), ring + unit + ragged tail (odd: no
            # multiple of the 16-byte vector either)
            for M in (5, 32, U * rows, 32 * rows, (32 + U) * rows + 37):
                out.append((dtype, M, {"sweep_short": 1, "sweep_unit": U}))
    return out


def _dyn_cases():
    out = []
    for dtype in (F32, F64):
        rows = _rows(dtype)
        for U in (4, 8, 16):
            for dyn in (1, 8):
                for M in (130, (32 + U) * rows + 37):
                    out.append((dtype, M, {"sweep_short": 1, "sweep_unit": U, "sweep_dyn": dyn}))
    return out


def _short_cases():
    out = []
    for dtype in (F32, F64):
        rows = _rows(dtype)
        for M in (5, 32, rows, rows + 3, 2 * rows, 2 * rows + 1, 3 * rows + 1, 4 * rows - 1):  # NCH 1, 2, 4 (three and four chunks)
            out.append((dtype, M, {}))
    return out


def _ph_cases():
    out = []
    for dtype in (F32, F64):
        for M in (20500, 40002):
            for pr in (0, 8 * _rows(dtype)):  # the fewest phases the LDS allows; phases of ONE 8-load unit
                out.append((dtype, M, {"phase_rows": pr} if pr else {}))
    return out


CASES_SWEEP = _gen_cases() + _dyn_cases() + _short_cases() + _ph_cases()
SWEEP_N = (1, 3, 5, 259)  # (259 where 8 MiB hold it: a phased f32 column of 40002 rows leaves 52, see ncols)


def _id(case):
    dtype, M, tunes = case[0], case[1], case[2]
    return "%s-%d-%s" % (np.dtype(dtype).name, M, "-".join("%s%d" % (k.replace("sweep_", ""), v) for k, v in tunes.items()) or "default")


@pytest.mark.parametrize("case", CASES_SWEEP, ids=_id)
def test_exact_integer_sweeps(D, cus, case):
    """(a): abs_corr equals the int64 reference EXACTLY and top_idx is the lexsort order (ties to the lower index), for every
    stand-alone body and unit size, with columns planted so that they tie across waves, workgroups, a wave's sequence and its store
    boundary.  n (the bound's chain length) is irrelevant here: integer partial sums make every order exact."""
    dtype, M, tunes = case
    for N0 in SWEEP_N:
        N = ncols(M, dtype, N0)
        for grid in ((0,) if N < 16 else (0, 1, 2)):
            t = dict(tunes)
            if grid:
                t["sweep_grid"] = grid
            p = sp.plan(M, N, dtype, cus, t)
            kern = p.sweep()
            A = int_dict(M, N, dtype, 7 * M + N)
            r = int_vec(M, M + N + grid)
            plant_ties(A, r, tie_columns(p, kern, N, p.sweep_grid))
            d = D(A, **t)
            check_config(d, p)
            check_sweep_exact(d, A, r)
            check_sweep_exact(d, A, int_vec(M, 3 * M + N))  # (a second residual: no planted ties, the c store alone)
            d.close()


# ------------------------------------------------------------------------------------------ (b) CStage boundaries
# waves that own 63, 64, 65, 128, 129 columns, and one wave with one column more than the others (257 on one workgroup)
STAGE_N = {1: (252, 256, 257, 260, 512, 516), 2: (504, 512, 513, 520, 1024, 1032)}
# k_sweep_short stores every 64 KS = 384 columns of a wave (csmp_kernels.hpp:709, :812-815): wave 0 owns 385 columns (one full store,
# then a flush of one), and every wave owns more than 384 with a ragged last group
STAGE_N_SHORT = {1: (1537, 1579), 2: (3073, 3155)}
CASES_STAGE = [(dtype, M) for dtype in (F32, F64) for M in (130, 1001)]


@pytest.mark.parametrize("dtype,M", CASES_STAGE)
@pytest.mark.parametrize("grid", [1, 2])
def test_cstage_boundaries_of_the_single_sweep(D, cus, dtype, M, grid):
    """(b): every entry of c, integer data, a wave's 64-column stores and the final flush of 63 / 0 / 1 columns (k_sweep_gen).  For
    M = 130 also k_sweep_short: at STAGE_N only its final flush runs (no wave reaches the 384 columns of its store), at STAGE_N_SHORT
    wave 0 makes one full store and flushes 1 column, or every wave stores once and flushes a ragged rest.  Two residuals per
    dictionary: one with ties planted by the twin's map (across the wave's store boundary among them), one without."""
    for N in STAGE_N[grid] + (STAGE_N_SHORT[grid] if M == 130 else ()):
        A0 = int_dict(M, N, dtype, M + N)
        for short in ((1, 0) if M == 130 else (1,)):
            t = {"sweep_grid": grid, "sweep_short": short}
            p = sp.plan(M, N, dtype, cus, t)
            assert p.sweep_grid == grid
            kern = p.sweep()
            assert kern[0] == ("k_sweep_gen" if short else "k_sweep_short")
            per_wave = [len(sp.wave_columns(sp.body_of(kern), b, w, N, grid, p.short_nch)) for b in range(grid) for w in range(4)]
            assert sum(per_wave) == N
            if short and N in STAGE_N[grid]:
                assert per_wave[0] == (63, 64, 65, 65, 128, 129)[STAGE_N[grid].index(N)] and max(per_wave) == per_wave[0], per_wave
            if N in STAGE_N_SHORT[grid] and not short:
                assert per_wave[0] > 384 and (N != STAGE_N_SHORT[grid][0] or per_wave == [385] + [384] * (4 * grid - 1)), per_wave
            A, r = A0.copy(order="F"), int_vec(M, N + grid)
            ties = tie_columns(p, kern, N, grid)
            assert len(ties) == 7 or per_wave[0] <= (64 if short else 384)  # (the two columns beside wave 0's first store are planted)
            plant_ties(A, r, ties)
            d = D(A, **t)
            check_config(d, p)
            check_sweep_exact(d, A, r)
            check_sweep_exact(d, A, int_vec(M, N + grid + 7))
            d.close()


def first_argmax(A, b):
    c = np.abs(exact(A, b))
    return int(np.argmax(c)), c  # (np.argmax: the first maximum)


@pytest.mark.parametrize("dtype,M", CASES_STAGE)
@pytest.mark.parametrize("grid", [1, 2])
def test_cstage_boundaries_of_the_tick_sweep(D, cus, dtype, M, grid):
    """(b) through k_tick (omp_batch on ONE pipeline, tick_grid 1 and 2, k = 1): the pick is the reference's first arg-max and the
    coefficient is <a_j, b> / |a_j|^2 -- the atom wins by its place in c, whichever store wrote it.  Signals: a random one; one
    whose two best columns tie on both sides of wave 0's store boundary (where wave 0 owns 64 columns or fewer: its last column and
    column N - 1); one whose two best columns tie across waves (column 1 and column N - 2)."""
    for N in STAGE_N[grid]:
        A = int_dict(M, N, dtype, 2 * M + N)
        t = {"pipelines": 1, "tick_grid": grid}
        p = sp.plan(M, N, dtype, cus, t)
        assert p.pipe_nblk(p.tick_grid) == grid and p.tick(True)[0] == "k_tick"
        w0 = sp.wave_columns("gen", 0, 0, N, grid)
        B = np.stack([int_vec(M, N + s) for s in range(3)], axis=1)
        t1 = [w0[63], w0[64]] if len(w0) > 64 else [w0[-1], N - 1]
        t2 = [1, N - 2]
        assert len(set(t1 + t2)) == 4
        plant_ties(A, B[:, 1], t1)
        plant_ties(A, B[:, 2], t2)
        assert first_argmax(A, B[:, 1])[0] == t1[0] and first_argmax(A, B[:, 2])[0] == 1  # (the planted pairs are the signals' maxima)
        assert first_argmax(A, B[:, 1])[1][t1[1]] == first_argmax(A, B[:, 1])[1][t1[0]]
        d = D(A, **t)
        check_config(d, p)
        bi, bv, bn = d.ctx.omp_batch(np.asfortranarray(B), 1, 0.0)
        for s in range(3):
            j, c = first_argmax(A, B[:, s])
            assert bn[s] == 1 and bi[0, s] == j, (N, s, bi[0, s], j)
            a = A[:, j].astype(F64)
            assert close(bv[:1, s], np.array([a @ B[:, s] / (a @ a)]))
        d.close()


# ------------------------------------------------------------------------------------------ (c) column probes of the shared passes
# The first MP coefficient of a signal is c at its arg-max: k_mp_group reduces the pass's partials with better(), reads
# c = cvec[m][bi] and logs (bi, c) (csmp_kernels.hpp:2910-2933; host/mp_batch.hpp:21-35 launches it after the shared pass).
# mp_batch with k = 1 therefore returns (arg-max, c[arg-max]) per member; k = 2 adds a second step on r - c a_j, whose output is
# merged by k_mp_emit's rule (ascending atoms, a repeated atom summed, an all-zero atom dropped).
CASES_SHARED_F32 = [(F32, M, 0) for M in (32, 64, 130, 256, 1001, 3000)]
CASES_SHARED_F64 = [(F64, M, U) for U in (4, 8, 16) for M in (130, 512, 1003, 1536, 3000)]
GROUPS_NARROW = (1, 2, 3, 4)
GROUPS_WIDE = (5, 6, 7, 8)  # (5 and 7: unequal halves, R = 3 / 4 with a masked entry in the second half)


def shared_sizes(dtype, M):
    """the group sizes of a dictionary: wide groups are Float32's alone (group_wide, host/dictionary.hpp:217-218)"""
    return GROUPS_NARROW + (GROUPS_WIDE if dtype == F32 else ())


# one test case per (dictionary, narrow sizes) and per (dictionary, ONE wide size): a wide pass has 64 waves to probe
CASES_SHARED = ([c + (GROUPS_NARROW,) for c in CASES_SHARED_F32 + CASES_SHARED_F64] +
                [c + ((size,),) for c in CASES_SHARED_F32 + CASES_SHARED_F64 for size in shared_sizes(c[0], c[1])[len(GROUPS_NARROW):]])


def shared_tunes(dtype, U, size, grid):
    t = {"pipelines": 3, "tick_grid": grid}
    if U:
        t["sweep_unit"] = U
    if size <= 4:
        t["group_max"] = size
    return t


def shared_N(dtype, M, size, grid):
    """columns so that a wave of the pass crosses its 64-column store where 8 MiB allow it"""
    streams = 8 if size > 4 else grid  # (a wide pass runs on wide_nblk / 2 = 8 streams at least)
    waves = streams * (8 if dtype == F32 else 4)
    return ncols(M, dtype, 64 * waves + 2 * waves + 3)  # (odd: the last pair of the Float32 body has ONE column)


def probe_columns(p, kern, N, nblk):
    body = sp.body_of(kern)
    cols = [0, 1, N - 2, N - 1]
    for b in range(nblk):
        for w in range(8 if body == "multi" else 4):
            wc = sp.wave_columns(body, b, w, N, nblk)
            if len(wc) > 64:
                cols += [wc[63], wc[64]]
    return [c for c in dict.fromkeys(cols) if 0 <= c < N]


def mp_reference(A, b, k):
    """MP on integer data, exactly (int64): the (atom, increment) log of k steps and what k_mp_emit makes of it"""
    Ai = A.astype(np.int64)
    r = b.astype(np.int64)
    log = []
    for _ in range(k):
        # what makes Float64 exact in ANY order: every partial sum of a column is below sum_i |a_ij r_i| < 2^53
        assert (np.abs(Ai).T @ np.abs(r)).max() < 2 ** 53
        c = Ai.T @ r
        j = int(np.argmax(np.abs(c)))
        log.append((j, int(c[j])))
        r = r - c[j] * Ai[:, j]
        assert np.abs(r).max() + 8 * abs(int(c[j])) < 2 ** 53  # (the update r - c a_j, fused or not)
    atoms = sorted({j for j, _ in log if any(v != 0 for jj, v in log if jj == j)})
    return atoms, [float(sum(v for jj, v in log if jj == j)) for j in atoms]


def run_shared(d, B, k):
    got = d.ctx.mp_batch(np.asfortranarray(B), k)
    alone = [d.ctx.mp(B[:, s], k) for s in range(B.shape[1])]
    for s, (i, v) in enumerate(alone):  # bit-equal to ctx.mp on that signal alone
        assert got[2][s] == len(i) and np.array_equal(got[0][:len(i), s], i) and np.array_equal(got[1][:len(i), s], v), (s, got[0][:, s], i)
    return got


@pytest.mark.parametrize("case", CASES_SHARED, ids=lambda c: "%s-%d-U%d-%s" % (np.dtype(c[0]).name, c[1], c[2], "narrow" if len(c[3]) > 1 else "wide%d" % c[3][0]))
@pytest.mark.parametrize("grid", [1, 2])
def test_shared_pass_column_probes(D, cus, case, grid):
    """(c) and the shared-pass part of (b): members b_s = g_s + t a_j with j on the edges of the column range and on both sides of
    every wave's 64-column store; among the members a zero signal and a one-atom signal (mp_batch runs with skipmask = 0 and no eps
    test, so these two do NOT switch a `live` bit off: their increments are zero and the pass goes on storing them; the only
    entries a pass masks here are those of the shorter half of wide 5 and 7 -- test_shared_pass_with_stopped_members below runs
    passes beside members that HAVE stopped).  Per member: idx is the reference's arg-max,
    val within the bound (n = image rows per lane + 6: the pass runs sweep_body_gen's chain per member), idx and val bit-equal to
    ctx.mp alone (k = 1 and k = 2).  Then the same schedules on integer data against the exact MP reference, two steps."""
    dtype, M, U, sizes = case
    g = np.random.default_rng(M + grid)
    for size in sizes:
        t = shared_tunes(dtype, U, size, grid)
        N = shared_N(dtype, M, size, grid)
        p = sp.plan(M, N, dtype, cus, t)
        assert p.sweep_group >= 1 and size <= max(p.group_wide, p.sweep_group), (size, p.sweep_group, p.group_wide)
        kern, streams = p.shared(size)
        n = sp.chain_length(p, kern)
        A = gauss_dict(M, N, dtype, M + N)
        A64 = A.astype(np.longdouble)
        cols = probe_columns(p, kern, N, streams)
        d = D(A, **t)
        check_config(d, p)
        nsig = max(size, 2)
        for c0 in range(0, len(cols), max(nsig - 2, 1)):
            B = np.zeros((M, nsig))
            want = [None] * nsig
            for s in range(nsig):
                if s == nsig - 1:
                    continue  # the zero signal (a pass of ONE member: the second group)
                j = cols[(c0 + s) % len(cols)]
                gs = g.standard_normal(M) if s != nsig - 2 else np.zeros(M)  # (s = nsig - 2: the one-atom signal)
                tt = 1.0 + 50.0 * float(np.max(np.abs(A.astype(F64).T @ gs)))
                B[:, s] = gs + tt * A[:, j].astype(F64)
                want[s] = j
            ref = np.asarray(A64.T @ B.astype(np.longdouble))
            got = run_shared(d, B, 1)
            for s in range(nsig):
                if want[s] is None:
                    assert got[2][s] == 0  # every increment of the zero signal is exactly zero: no entry
                    continue
                bd = bound(A, B[:, s], n)
                a = np.abs(ref[:, s])
                j = int(np.argmax(a))
                assert j == want[s] and a[j] - np.max(np.delete(a, j)) > 2 * float(np.max(bd)), "the probe's margin"
                assert got[2][s] == 1 and got[0][0, s] == j, (size, s, got[0][0, s], j)
                assert abs(np.longdouble(got[1][0, s]) - ref[j, s]) <= bd[j], (size, s, j)
            run_shared(d, B, 2)
        d.close()
        # the tolerance-free pass: integer data, two steps, the exact reference
        Ai = int_dict(M, N, dtype, 5 * M + N)
        di = D(Ai, **t)
        Bi = np.stack([int_vec(M, N + s) + 64.0 * Ai[:, cols[s % len(cols)]] for s in range(nsig)], axis=1)
        Bi[:, nsig - 1] = 0.0
        got = run_shared(di, Bi, 2)
        for s in range(nsig):
            atoms, vals = mp_reference(Ai, Bi[:, s], 2)
            assert got[2][s] == len(atoms) and list(got[0][:len(atoms), s]) == atoms and list(got[1][:len(atoms), s]) == vals, (size, s)
        di.close()


CASES_STOPPED = [(F32, 1001, 4), (F32, 1001, 7), (F32, 3000, 5), (F64, 1003, 4), (F64, 130, 3)]


@pytest.mark.parametrize("dtype,M,nsig", CASES_STOPPED)
def test_shared_pass_with_stopped_members(D, cus, oracle, dtype, M, nsig):
    """A shared pass beside members whose `live` bit is off (host/omp.hpp: done & skipmask): grouped omp_batch (pipelines = 3) with
    eps > 0 on exactly sparse signals of 1, 2, .. atoms and k = 4 -- member s stops after s + 1 atoms (STOP_EPS) while the others go on,
    so the passes of steps 2 .. 4 run with one, two, .. members masked, in both halves of a wide group.  Every member: support and
    coefficients are the oracle's, and the bits those of the one-pipeline schedule."""
    k, eps = 4, 1e-8  # (the signals are exact combinations of +-1: a residual of 1e-13 at most once the support is found, above 0.5 before)
    N = ncols(M, dtype, 600)
    A = gauss_dict(M, N, dtype, M + 11)
    p = sp.plan(M, N, dtype, cus, {"pipelines": 3})
    assert p.sweep_group == 4 and max(p.group_wide, p.sweep_group) >= min(nsig, 8 if dtype == F32 else 4)
    assert p.shared(nsig)[0][0] == ("k_sweep_wide" if nsig > 4 else "k_sweep_multi" if dtype == F32 else "k_sweep_multi_w4")
    Y = np.asfortranarray(np.stack([planted(A, 1 + s % k, 50 + s, 0.0) for s in range(nsig)], axis=1))
    d = D(A, pipelines=3)
    check_config(d, p)
    got = d.ctx.omp_batch(Y, k, eps)
    d.ctx.tune("pipelines", 1)
    one = d.ctx.omp_batch(Y, k, eps)
    assert all(np.array_equal(x, y) for x, y in zip(got, one))
    for s in range(nsig):
        ref = oracle.omp(A, Y[:, s], k, eps)
        assert len(ref[0]) == 1 + s % k, (s, ref[0])  # the member stopped where it was meant to
        assert got[2][s] == len(ref[0]) and np.array_equal(got[0][:got[2][s], s], ref[0]) and close(got[1][:got[2][s], s], ref[1]), s


# ------------------------------------------------------------------------------------------ (d) bits across U and across bodies
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("M", [130, 1003, 3000])
def test_bits_across_unit_sizes_and_bodies(D, cus, dtype, M):
    """(d): in sweep_body_gen a lane's chain runs over the image's chunks in increasing order whatever U is (t = cb * U + u,
    csmp_kernels.hpp:402; rows past Mv add a * 0), and so do sweep_body_dyn (:1030 ff.), the tick kernel (the same bodies) and
    sweep_body_multi_w4 (:2451 ff.): c, top-k and omp results are bit-equal across sweep_unit 4 / 8 / 16.  DESIGN promises the same
    between the short and the one-column body (csmp_kernels.hpp:673) and between the dynamic and the static split.
    The Float32 shared pass (sweep_body_multi) has one unit size only: nothing to compare."""
    N = ncols(M, dtype, 523)
    A = gauss_dict(M, N, dtype, M + 1)
    g = np.random.default_rng(M)
    r = g.standard_normal(M)
    B = np.asfortranarray(g.standard_normal((M, 4)) + 3.0 * A[:, [5, N - 1, 17, N // 2]].astype(F64))
    outs = {}
    for U in (4, 8, 16):
        for variant, extra in (("gen", {"sweep_short": 1}), ("dyn", {"sweep_short": 1, "sweep_dyn": 1}), ("auto", {})):
            t = dict(extra, sweep_unit=U)
            p = sp.plan(M, N, dtype, cus, t)
            d = D(A, **t)
            check_config(d, p)
            res = [d.ctx.sweep(r, topk=7), d.ctx.omp(B[:, 0], 6, 0.0)]
            if variant != "auto":
                d.ctx.tune("pipelines", 1)  # the tick kernel on this body
                res.append(d.ctx.omp_batch(B, 6, 0.0))
            if variant == "gen" and dtype == F64:
                d.ctx.tune("pipelines", 3)  # k_sweep_multi_w4<double, U, 4> and <., U, 2>
                res.append(d.ctx.mp_batch(B, 5))
                res.append(d.ctx.mp_batch(np.asfortranarray(B[:, :2]), 5))
            outs[(variant, U)] = res
            d.close()

    def same(x, y):
        return all(np.array_equal(a, b) for u, v in zip(x, y) for a, b in zip(u, v))
    for variant in ("gen", "dyn", "auto"):
        for U in (8, 16):
            assert same(outs[(variant, U)], outs[(variant, 4)]), (variant, U)
    for U in (4, 8, 16):
        assert same(outs[("dyn", U)][:3], outs[("gen", U)][:3]), ("dyn against static", U)
        assert same(outs[("auto", U)][:2], outs[("gen", U)][:2]), ("the automatic body (short where M <= 4 chunks) against gen", U)
    # against the reference, once: the bound with n = image rows per lane + 6 at the LARGEST image (U = 16 pads most)
    p = sp.plan(M, N, dtype, cus, {"sweep_short": 1, "sweep_unit": 16})
    ref = np.abs(np.asarray(A.astype(np.longdouble).T @ r.astype(np.longdouble)))
    err = np.abs(outs[("gen", 16)][0][0].astype(np.longdouble) - ref)
    assert np.all(err <= bound(A, r, sp.chain_length(p, p.sweep()))), float(err.max())


# ------------------------------------------------------------------------------------------ (e) the forward-regression matrix
# (dtype, M, tunes): fr_config yields <16, true> (with sweep_unit 16 also for NQ = -1 / 1), <8, true>, and the predicated <4, false>
# for a chunk count that neither block tiles (2304 = 9 chunks f32, 1152 f64) and for a ragged M.  NQ = -1 and 1: fr; NQ = 2: srr's
# replacement step (a backward and a forward correction pending, Stepwise::pass_of, host/twostage.hpp:436-445).  NQ = 0: the FIRST
# pass of srr after an oblivious acquisition (initialization = 1) -- srr_impl leaves rho_ready = true and nothing pending
# (host/twostage.hpp:680-682), and the loop's first iteration (maxiter = 4k >= 1) opens with launch_fr_pass(pass_of(0)) in
# forward_backward (:507) or forward (:471): nq = pend.size() = 0 (:439), whatever the data.
CASES_FR = [(F32, 4096, {"sweep_unit": 16}), (F32, 2048, {}), (F32, 2304, {}), (F32, 1001, {}),
            (F64, 2048, {"sweep_unit": 16}), (F64, 1024, {}), (F64, 1152, {}), (F64, 1003, {})]


def planted(A, k, seed, noise):
    g = np.random.default_rng(seed)
    M, N = A.shape
    b = A[:, g.choice(N, k, replace=False)].astype(F64) @ g.choice([-1.0, 1.0], k)
    e = g.standard_normal(M)
    return b + e * (noise / np.linalg.norm(e))


@pytest.mark.parametrize("case", CASES_FR, ids=_id)
def test_forward_regression_matrix(D, cus, oracle, case):
    """(e): selection order, support and coefficients of fr / srr / fr_batch against the oracle on every block form of k_fr_sweep and
    k_tick_fr.  Where the tick has no LDS form for M (a predicated block: batch_schedule, host/forward.hpp:252-256) fr_batch solves
    one signal at a time -- the twin's fr_tick() is None -- and the results are still the oracle's."""
    dtype, M, tunes = case
    N, k = ncols(M, dtype, 500), 8
    A = gauss_dict(M, N, dtype, 3 * M + 1)
    p = sp.plan(M, N, dtype, cus, tunes)
    want_full = M % (64 * p.vec) == 0 and (M // (64 * p.vec)) % 8 == 0
    for nq in (-1, 0, 1, 2):
        kern = p.fr_pass(nq)
        assert kern != "tall" and kern[3] == want_full, kern
        assert kern[2] == (4 if not want_full else 16 if (tunes.get("sweep_unit") == 16 or nq == 2) and (M // (64 * p.vec)) % 16 == 0 else 8)
    assert (p.fr_tick(True) is None) == (not want_full)
    d = D(A, **tunes)
    check_config(d, p)
    for seed in range(2):
        y = planted(A, k, seed, 0.05)
        ref = oracle.fr(A, y, k)
        got = d.ctx.fr(y, k, 0.0, 0.0)
        assert np.array_equal(got[2], ref[2]), "fr selection order"
        assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
        ys = planted(A, k + 2, 10 + seed, 0.2)  # two atoms more than srr may keep: the replacement loop works
        for init in (1, 2):
            rs = oracle.srr(A, ys, k, 1e-12, -1, init, 1)
            gs = d.ctx.srr(ys, k, 1e-12, -1, init, 1)
            assert np.array_equal(gs[0], rs[0]) and close(gs[1], rs[1]) and gs[2] == rs[2], (init, gs[2], rs[2])
            assert gs[2] >= 1  # (an iteration ran: with init = 1 its first pass is the NQ = 0 one)
    for nsig in (3, 5):
        Y = np.asfortranarray(np.stack([planted(A, k, 20 + s, 0.05) for s in range(nsig)], axis=1))
        bi, bv, bn = d.ctx.fr_batch(Y, k, 0.0, 0.0)
        for s in range(nsig):
            r3 = oracle.fr(A, Y[:, s], k)
            assert bn[s] == len(r3[0]) and np.array_equal(bi[:bn[s], s], r3[0]) and close(bv[:bn[s], s], r3[1]), (nsig, s)


# ------------------------------------------------------------------------------------------ the tick kernel's instantiations
CASES_TICK = ([(dtype, 1003, {"sweep_unit": U, "sweep_dyn": dyn}) for dtype in (F32, F64) for U in (4, 8, 16) for dyn in (0, 1)] +
              [(dtype, 20500, {}) for dtype in (F32, F64)])


@pytest.mark.parametrize("case", CASES_TICK, ids=_id)
def test_tick_kernel_on_every_body(D, cus, oracle, case):
    """k_tick<TA, U, PH, STEADY, DYN> on one pipeline of three signals (five signals, k = 4: fill, steady and drain ticks): supports
    and coefficients against the oracle, and on integer data the first pick against the exact arg-max"""
    dtype, M, tunes = case
    t = dict(tunes, pipelines=1)
    N = ncols(M, dtype, 300)
    A = gauss_dict(M, N, dtype, M + 3)
    p = sp.plan(M, N, dtype, cus, t)
    kern = p.tick(True)
    assert kern[3] == (M > 20000) and kern[5] == bool(tunes.get("sweep_dyn"))
    d = D(A, **t)
    check_config(d, p)
    eps = float(np.finfo(dtype).eps)
    Y = np.asfortranarray(np.stack([planted(A, 4, 30 + s, 0.05) for s in range(5)], axis=1))
    bi, bv, bn = d.ctx.omp_batch(Y, 4, eps)
    for s in range(5):
        ref = oracle.omp(A, Y[:, s], 4, eps)
        assert bn[s] == len(ref[0]) and np.array_equal(bi[:bn[s], s], ref[0]) and close(bv[:bn[s], s], ref[1]), s
    d.close()
    Ai = int_dict(M, N, dtype, M + 4)
    di = D(Ai, **t)
    Bi = np.asfortranarray(np.stack([int_vec(M, 40 + s) for s in range(5)], axis=1))
    bi, bv, bn = di.ctx.omp_batch(Bi, 1, 0.0)
    for s in range(5):
        assert bn[s] == 1 and bi[0, s] == first_argmax(Ai, Bi[:, s])[0], s


# ------------------------------------------------------------------------------------------ what the tables reach, per the twin
def reached(cus=256):
    """the kernel names the case tables above launch, per the twin (tests/test_sweep_plan_static.py compares them with the code object)"""
    names = set()
    for dtype, M, tunes in CASES_SWEEP:
        for N0 in SWEEP_N:
            N = ncols(M, dtype, N0)
            names.add(sp.kernel_name(sp.plan(M, N, dtype, cus, tunes).sweep()))
    for dtype, M, tunes in CASES_TICK:
        p = sp.plan(M, ncols(M, dtype, 300), dtype, cus, dict(tunes, pipelines=1))
        names |= {sp.kernel_name(p.tick(True)), sp.kernel_name(p.tick(False))}
    for dtype, M, U in CASES_SHARED_F32 + CASES_SHARED_F64:
        for grid in (1, 2):
            for size in shared_sizes(dtype, M):
                p = sp.plan(M, shared_N(dtype, M, size, grid), dtype, cus, shared_tunes(dtype, U, size, grid))
                assert p.sweep_group >= 1 and size <= max(p.group_wide, p.sweep_group), (dtype, M, U, size)
                names.add(sp.kernel_name(p.shared(size)[0]))
    for dtype, M, nsig in CASES_STOPPED:
        names.add(sp.kernel_name(sp.plan(M, ncols(M, dtype, 600), dtype, cus, {"pipelines": 3}).shared(nsig)[0]))
    for dtype, M, tunes in CASES_FR:
        p = sp.plan(M, ncols(M, dtype, 500), dtype, cus, tunes)
        names |= {sp.kernel_name(p.fr_pass(nq)) for nq in (-1, 0, 1, 2)}  # (0: srr with initialization = 1, see CASES_FR)
        for first in (True, False):
            if p.fr_tick(first):
                names.add(sp.kernel_name(p.fr_tick(first)))
    return names
