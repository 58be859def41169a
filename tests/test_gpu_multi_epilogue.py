"""GPU tests (pytest -m gpu) of the shared Float32 pass (sweep_body_multi under k_sweep_multi / k_sweep_wide) after its epilogue
became one transposing butterfly per set of (member, column) values and its whole-unit columns lost the row clamp:

  both load paths   M = 1024, 2048, 4096 (whole units, nunit = 1, 2, 4: the unclamped instantiation) and M = 1000, 1028, 4092 (ragged
                    rows: the clamped one), N = 1, 2, 3, 7, 1023, 2050 on grids of 16 and 32 workgroups (waves with no pair, one pair,
                    several; an odd N discards the second column of its last pair), groups of 1 .. 8 members (narrow R = 1 .. 4, wide
                    3 + 2, 3 + 3, 4 + 3, 4 + 4): omp_batch gives the bits of one pipeline of single signals;
  every c           mp_batch column probes on integer data: every member's (atom, coefficient) is the exact int64 reference and
                    bit-equal to mp on that signal alone, with the probe on every column (N <= 7) or on the columns the twin names:
                    both parities of a pair, the pairs on both sides of the 16- and 32-pair stores of a wave, the edges;
  members that leave  a zero signal, a one-atom signal, an exactly 2-sparse one and a duplicate in one group: the live mask changes
                    between passes, the outputs (prefilled) are those of one pipeline, bit for bit, also where nothing is written;
  planted ties      equal |c| in the two columns of ONE pair, in two pairs of a wave, in two waves, in two workgroups, at the first
                    and the last column, for every member of R = 3 and R = 4 (narrow and wide) and both signs of c: the LOWEST index.

The helpers are those of tests/test_gpu_sweep_matrix.py and tests/test_gpu_wide_groups.py; integer data makes Float64 exact in any
order (entries in [-8, 8], signals small enough that every partial sum stays below 2^53: mp_reference asserts it), so no tolerance
appears anywhere in this file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_plan as sp  # noqa: E402
import test_gpu_sweep_matrix as matrix  # noqa: E402
import test_gpu_wide_groups as wg  # noqa: E402
from test_gpu_sweep_matrix import D, cus  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu

F32 = np.float32
MS_WHOLE = (1024, 2048, 4096)
MS_RAGGED = (1000, 1028, 4092)
NS = (1, 2, 3, 7, 1023, 2050)
GRIDS = (16, 32)
SIZES = (1, 2, 3, 4, 5, 6, 7, 8)


def tunes(size, grid):
    t = {"pipelines": 3, "tick_grid": grid}
    if size <= 4:
        t["group_max"] = size
    return t


def kernel_of(M, N, cus, size, grid):
    """(kernel, column streams) of a group of `size` by the twin; the pass is the Float32 pair body with R = the larger half"""
    p = sp.plan(M, N, F32, cus, tunes(size, grid))
    kern, streams = p.shared(size)
    assert kern[0] == ("k_sweep_wide" if size > 4 else "k_sweep_multi") and kern[3] == (size if size <= 4 else (size + 1) // 2)
    return p, kern, streams


# ------------------------------------------------------------------------------------------ both load paths: omp_batch
def planted_signals(A, k, nsig, seed):
    g = np.random.default_rng(seed)
    M, N = A.shape
    cols = []
    for s in range(nsig):
        S = g.choice(N, size=min(k, N), replace=False)
        cols.append(A[:, S].astype(np.float64) @ g.choice([-1.0, 1.0], size=len(S)) + 5e-3 * g.standard_normal(M))
    return np.asfortranarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("M", MS_WHOLE + MS_RAGGED)
def test_groups_of_one_to_eight_give_the_bits_of_one_pipeline(D, cus, M, grid):
    eps = float(np.finfo(F32).eps)
    for N in NS:
        k = min(3, N)
        A = matrix.gauss_dict(M, N, F32, M + N)
        d = D(A)
        assert d.ctx.sweep_config()["group_max"] == 4 and d.ctx.sweep_config()["group_wide"] == 8
        B = planted_signals(A, k, max(SIZES), M + 7 * N + grid)
        ref = wg.run(d, B, k, eps, pipelines=1)
        for size in SIZES:
            kernel_of(M, N, cus, size, grid)
            got = wg.run(d, np.asfortranarray(B[:, :size]), k, eps, **tunes(size, grid))
            assert wg.same(got, [x[..., :size] for x in ref]), (N, size)
        d.close()


# ------------------------------------------------------------------------------------------ every c: mp_batch column probes
def probe_columns(N, streams):
    """every column of a small N; else the edges and, for the first and the last wave that own them, both columns of the pairs
    0, 1, 15, 16, 31, 32 of the wave's sequence (a set of four stores every 16 pairs, a set of two every 32)"""
    if N <= 8:
        return list(range(N))
    cols = [0, 1, 2, 3, N - 2, N - 1]
    for b, w in ((0, 0), (0, 5), (streams - 1, 7)):
        wc = sp.wave_columns("multi", b, w, N, streams)
        for pair in (0, 1, 15, 16, 31, 32):
            cols += wc[2 * pair:2 * pair + 2]
    return [c for c in dict.fromkeys(cols) if 0 <= c < N][:24]


def mp_exact(A64, absA, b, k):
    """matrix.mp_reference with the products in Float64 (BLAS): on this integer data every partial sum of a column is an integer
    below 2^53 (asserted, as there), so the Float64 product is the int64 one in ANY order -- and a fraction of its time"""
    r = b.copy()
    log = []
    for _ in range(k):
        assert (absA.T @ np.abs(r)).max() < 2 ** 53
        c = A64.T @ r
        j = int(np.argmax(np.abs(c)))  # (the first maximum)
        log.append((j, c[j]))
        r = r - c[j] * A64[:, j]
        assert np.abs(r).max() + 8 * abs(c[j]) < 2 ** 53
    atoms = sorted({j for j, _ in log if any(v != 0 for jj, v in log if jj == j)})
    return atoms, [float(sum(v for jj, v in log if jj == j)) for j in atoms]


@pytest.mark.parametrize("grid", GRIDS + (2,))  # (2: 16 waves, so that a wave of N = 2050 crosses its 16- and 32-pair stores)
@pytest.mark.parametrize("M", (1024, 4096, 1000, 4092))
def test_every_member_reads_every_probed_c(D, cus, M, grid):
    """members b_s = noise_s + 64 a_j, j running over the probe columns; among them the one-atom signal (no noise) and the zero
    signal.  Two steps of mp_batch: the second step's increment is the c of the first step's residual at the atom picked."""
    for N in NS if grid != 2 else (1023, 2050):
        A = matrix.int_dict(M, N, F32, 3 * M + N)
        A64 = A.astype(np.float64)
        absA = np.abs(A64)
        d = D(A)
        for size in SIZES if grid != 2 else (1, 3, 4):
            p, kern, streams = kernel_of(M, N, cus, size, grid)
            for key, v in tunes(size, grid).items():
                d.ctx.tune(key, v)
            matrix.check_config(d, p)
            cols = probe_columns(N, streams)
            for c0 in range(0, len(cols), size):
                B = np.zeros((M, size))
                for s in range(size):
                    j = cols[(c0 + s) % len(cols)]
                    B[:, s] = 64.0 * A64[:, j] + (matrix.int_vec(M, N + 31 * s + c0) if s != size - 2 else 0.0)  # (size - 2: one atom)
                if size >= 3:
                    B[:, size - 1] = 0.0  # the zero signal
                got = matrix.run_shared(d, B, 2)  # bit-equal to ctx.mp on every signal alone (asserted there)
                for s in range(size if N <= 8 or c0 == 0 else 0):  # (the exact reference too: every call of a small N, else one a size)
                    atoms, vals = mp_exact(A64, absA, B[:, s], 2)
                    assert got[2][s] == len(atoms) and list(got[0][:len(atoms), s]) == atoms and list(got[1][:len(atoms), s]) == vals, (N, size, s)
            for key in tunes(size, grid):
                d.ctx.tune(key, 0)
        d.close()


# ------------------------------------------------------------------------------------------ members that leave
@pytest.mark.parametrize("M", (1024, 1000))
@pytest.mark.parametrize("size", (3, 4, 6, 7, 8))
def test_members_that_leave_keep_their_outputs(cs, cus, M, size):
    """grouped omp_batch on the device with eps > 0: the zero signal and the one-atom signal stop after the first step, the 2-sparse one
    after two, the others run k = 4 steps, so the live mask of the group's pass changes from pass to pass.  idx / val / nnz are
    PREFILLED: what a stopped member's pass would write were it not masked shows as a difference from one pipeline of single signals."""
    import torch
    N, k, eps = 1023, 4, 1e-8
    A = matrix.gauss_dict(M, N, F32, M + size)
    g = np.random.default_rng(size)

    def full():
        S = g.choice(N, size=k, replace=False)
        return A[:, S].astype(np.float64) @ g.choice([-1.0, 1.0], size=k) + 5e-3 * g.standard_normal(M)
    # members 0, 1, 2: the zero signal, one atom, exactly 2-sparse; then signals that go on; the LAST member repeats the one before it
    # (size 3: the three that leave and no other -- the pass returns early once all have stopped); in a wide group (first half
    # (size + 1) / 2 members) the first member of the second half is one atom too, so both halves lose members
    cols = [np.zeros(M), A[:, N // 3].astype(np.float64), A[:, [5, N - 2]].astype(np.float64) @ np.array([1.0, -1.0])]
    cols += [full() for _ in range(size - 3)]
    if size > 4:
        cols[(size + 1) // 2] = A[:, N // 2 + 1].astype(np.float64)
    if size >= 4:
        cols[size - 1] = cols[size - 2].copy()  # the duplicate (size 4: of the 2-sparse signal)
    B = torch.tensor(np.stack(cols, axis=0), dtype=torch.float64, device="cuda").contiguous()
    kernel_of(M, N, cus, size, 16)
    d = cs.Dictionary(A)
    outs = []
    for t in ({"pipelines": 1}, tunes(size, 16)):
        idx = torch.full((size, k), -7, dtype=torch.int64, device="cuda")
        val = torch.full((size, k), -7.5, dtype=torch.float64, device="cuda")
        nnz = torch.full((size,), -7, dtype=torch.int64, device="cuda")
        for key, v in t.items():
            d.ctx.tune(key, v)
        d.ctx.omp_batch_device(B, k, eps, idx, val, nnz)
        d.ctx.sync()
        for key in t:
            d.ctx.tune(key, 0)
        outs.append((idx.cpu().numpy(), val.cpu().numpy(), nnz.cpu().numpy()))
    d.close()
    one, grouped = outs
    assert all(np.array_equal(x, y) for x, y in zip(one, grouped)), (one, grouped)
    nnz = one[2]
    assert nnz[0] <= 1 and nnz[1] == 1 and nnz[2] == 2, nnz  # the members that left, where they were meant to
    assert size != 4 or nnz[3] == 2
    assert size < 6 or nnz[size - 2] == k and nnz[size - 1] == k  # ... beside members that went on, and the duplicate with them
    assert size < 5 or nnz[(size + 1) // 2] == 1


# ------------------------------------------------------------------------------------------ planted ties
def tie_sets(N, streams):
    """(name, columns) of the planted ties by the twin's map of a stream's waves; the lowest column has to win.  Where two parities meet,
    the LOWER column is the odd one: the lane rows of the two parities keep their own first maximum, and better() must order them."""
    w1 = sp.wave_columns("multi", 0, 1, N, streams)
    w5 = sp.wave_columns("multi", 0, 5, N, streams)
    wl = sp.wave_columns("multi", streams - 1, 2, N, streams)
    assert len(w1) >= 6 and len(w5) >= 4 and len(wl) >= 4
    return [("one pair", [w1[2], w1[3]]),
            ("two pairs of a wave", [w1[1], w1[4]]),          # odd column of pair 0, even column of pair 2
            ("two pairs of a wave, same parity", [w1[3], w1[5]]),
            ("two waves", [w1[3], w5[0], w5[1]]),               # (w5's pair lies below w1[3]: the other wave wins)
            ("two workgroups", [w1[1], wl[0], wl[3]]),
            ("first and last", [0, N - 1])]


@pytest.mark.parametrize("M", (1024, 1000))
def test_planted_ties_select_the_lowest_index(D, cus, M):
    N, grid = 1023, 16
    A0 = matrix.int_dict(M, N, F32, 17 * M)
    pattern = np.where(np.random.default_rng(M).integers(0, 2, size=M) > 0, 1.0, -1.0)
    # every member's signal has the SAME signs and its own magnitudes: the planted columns reach 8 sum |r|, the largest |c| there is,
    # for all of them at once, and every member's coefficient is its own
    B8 = np.stack([pattern * (1.0 + np.abs(matrix.int_vec(M, 100 + s))) for s in range(8)], axis=1)
    for size in (3, 4, 6, 8, 5, 7):
        _, _, streams = kernel_of(M, N, cus, size, grid)
        for name, cols in tie_sets(N, streams):
            A = A0.copy(order="F")
            matrix.plant_ties(A, pattern, cols)
            d = D(A, **tunes(size, grid))
            C = matrix.exact(A, B8)  # int64: c of every column and member
            a = np.abs(C)
            assert all(np.count_nonzero(a[:, s] == a[:, s].max()) == len(set(cols)) for s in range(8)), (name, "the planted columns tie at the top, and only they")
            j = min(cols)
            for sign in (1.0, -1.0):
                got = matrix.run_shared(d, np.asfortranarray(sign * B8[:, :size]), 1)
                for s in range(size):
                    assert got[2][s] == 1 and got[0][0, s] == j and got[1][0, s] == sign * float(C[j, s]), (name, size, s, sign, got[0][0, s], j)
            d.close()
