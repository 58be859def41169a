"""GPU parity tests (pytest -m gpu) of csmp_omp_batch's grouped scheduler: each pipeline's three slots hold GROUPS of up to four
signals, and one launch (k_sweep_multi) computes c = A'r for every member of a group in ONE pass over the dictionary.  Every
signal keeps its own arithmetic, so the grouped runs (pipelines 0 = automatic and 3 = forced) must give the bits of one pipeline
of single signals (pipelines 1): supports, coefficients and counts, signals that stop on eps at different steps included.  Also the
phased sweep of a tall residual on the grid of two pipelines side by side (its per-wave LDS partials are sized for that grid)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


def close(v, ref, tol=1e-9):
    return np.allclose(v, ref, rtol=tol, atol=tol * (float(np.max(np.abs(ref))) if len(ref) else 0.0))


def dictionary(cs, M, N, dtype, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(torch.float32 if dtype == np.float32 else torch.float64)
    return At, np.asfortranarray(At.cpu().numpy().T)


def signals(cs, A, k, nsig, seed, stops=False):
    """planted k-sparse signals plus noise; stops: a zero signal, a signal equal to one atom, an exactly 2-sparse signal (eps-stops
    at different steps) and a duplicate of another signal among them"""
    rng = np.random.default_rng(seed)
    m = A.shape[1]
    cols = []
    for _ in range(nsig):
        xs = cs.sparse_vector(m, k, rng=rng)
        cols.append(cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=rng))
    if stops and nsig >= 4:
        cols[1] = np.zeros(A.shape[0])
        cols[2] = A[:, m // 3].astype(np.float64)
        cols[3] = cols[0].copy()
        if nsig >= 7:
            xs = cs.sparse_vector(m, 2, rng=rng)
            cols[5] = A[:, xs.nzind].astype(np.float64) @ xs.nzval  # exactly 2-sparse: stops after two steps
    return np.asfortranarray(np.stack(cols, axis=1))


def runs(d, B, k, eps, modes=(1, 3, 0)):
    out = {}
    for mode in modes:
        d.ctx.tune("pipelines", mode)
        out[mode] = d.ctx.omp_batch(B, k, eps)
    d.ctx.tune("pipelines", 0)
    return out


def assert_same(out, ref_mode=1):
    for mode, got in out.items():
        for a, b in zip(out[ref_mode], got):
            assert np.array_equal(a, b), mode


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [65536, 7920, 3000])
def test_grouped_scheduler_gives_the_bits_of_one_pipeline(cs, oracle, dtype, N):
    M, k = 4096, 6
    eps = float(np.finfo(dtype).eps)
    At, A = dictionary(cs, M, N, dtype, 7 + N)
    d = cs.Dictionary(At)
    assert d.ctx.sweep_config()["group_max"] == 4
    for nsig in (1, 2, 5, 7, 13, 20, 25):
        B = signals(cs, A, k, nsig, nsig + N, stops=True)
        out = runs(d, B, k, eps)
        assert_same(out)
        if nsig == 7:  # a few against the oracle: the stopped signals and a planted one
            idx, val, nnz = out[3]
            for s in (0, 1, 2, 5):
                ref = oracle.omp(A, B[:, s], k, eps)
                assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]), s
                assert close(val[:nnz[s], s], ref[1]), s
    d.close()


@pytest.mark.parametrize("group_max", [1, 2, 3])
def test_grouped_scheduler_smaller_groups(cs, group_max):
    """csmp_tune(group_max): groups of at most 1, 2 or 3 signals -- the same bits"""
    M, N, k, nsig = 4096, 3000, 5, 11
    At, A = dictionary(cs, M, N, np.float32, 11)
    d = cs.Dictionary(At)
    B = signals(cs, A, k, nsig, 5, stops=True)
    ref = runs(d, B, k, EPS32, modes=(1,))[1]
    d.ctx.tune("group_max", group_max)
    assert d.ctx.sweep_config()["group_max"] == group_max
    got = runs(d, B, k, EPS32, modes=(3,))[3]
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    d.close()


def test_grouped_scheduler_where_two_images_fit(cs, oracle):
    """9000 rows of f32: the LDS holds two residual images beside the scratch (group_max 2)"""
    M, N, k = 9000, 4000, 6
    At, A = dictionary(cs, M, N, np.float32, 3)
    d = cs.Dictionary(At)
    assert d.ctx.sweep_config()["group_max"] == 2
    for nsig in (2, 7, 13):
        B = signals(cs, A, k, nsig, 40 + nsig, stops=True)
        out = runs(d, B, k, EPS32)
        assert_same(out)
    idx, val, nnz = out[0]
    for s in (0, 4):
        ref = oracle.omp(A, B[:, s], k, EPS32)
        assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]), s
        assert close(val[:nnz[s], s], ref[1]), s
    d.close()


def test_grouped_scheduler_full_size(cs, oracle):
    """BASELINE configs[1] at its real size (4096 x 65536 f32, k = 256): 20 signals through the automatic choice (the grouped
    scheduler, groups of four) bit for bit as one pipeline of single signals, and two of them against the oracle"""
    import os
    M, N, k, nsig = 4096, 65536, 256, 20
    At, A = dictionary(cs, M, N, np.float32, 1234)
    d = cs.Dictionary(At)
    assert d.ctx.sweep_config()["group_max"] == 4
    B = signals(cs, A, k, nsig, 99)
    out = runs(d, B, k, EPS32, modes=(1, 0))
    assert_same(out)
    idx, val, nnz = out[0]
    nt = max(1, min(16, os.cpu_count() or 1))
    for s in (0, 13):
        ref = oracle.omp(A, B[:, s], k, EPS32, nthreads=nt)
        assert nnz[s] == len(ref[0]) == k and np.array_equal(idx[:, s], ref[0]), s
        assert close(val[:, s], ref[1], 1e-6), s
    d.close()


@pytest.mark.parametrize("N", [7920, 16384])
def test_phased_sweep_on_the_pair_grid(cs, oracle, N):
    """M = 32768 rows f32: the residual is staged in phases (sweep_body_ph) whose per-wave partials sit in the LDS.  Two pipelines
    side by side launch it on kPairTickGrid workgroups; the partials must be sized for that grid too (they were not for these N)."""
    M, k, nsig = 32768, 4, 3
    At, A = dictionary(cs, M, N, np.float32, N)
    d = cs.Dictionary(At)
    assert d.ctx.sweep_config()["phases"] > 1 and d.ctx.sweep_config()["group_max"] == 0
    B = signals(cs, A, k, nsig, N + 1)
    out = runs(d, B, k, EPS32, modes=(1, 2, 0))
    assert_same(out)
    idx, val, nnz = out[2]
    ref = oracle.omp(A, B[:, 0], k, EPS32)
    assert nnz[0] == len(ref[0]) and np.array_equal(idx[:nnz[0], 0], ref[0])
    assert close(val[:nnz[0], 0], ref[1])
    d.close()
