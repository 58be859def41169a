"""GPU parity tests (pytest -m gpu) of the shared sweep's workgroup mapping (k_sweep_multi on Float32: eight waves per workgroup,
two per SIMD, a pair of columns per wave at a time; Float64 keeps the four-wave body).  The grouped scheduler (pipelines = 3,
groups capped by group_max so that every group size R = 1 .. 4 runs) must give the bits of one pipeline of single signals
(pipelines = 1) where the grid holds fewer column pairs than waves, for odd column counts (a last pair of one column), for f32
and f64, for images of 8 and of 12 chunks of 256 rows, for the two-image shape, and with members that stop at different steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def dictionary(M, N, dtype, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(torch.float32 if dtype == np.float32 else torch.float64)
    return At, np.asfortranarray(At.cpu().numpy().T)


def signals(cs, A, k, nsig, seed):
    """planted k-sparse signals plus noise, with a zero signal, one atom and a duplicate among them (eps-stops at steps 0 and 1)"""
    rng = np.random.default_rng(seed)
    m = A.shape[1]
    cols = []
    for _ in range(nsig):
        xs = cs.sparse_vector(m, k, rng=rng)
        cols.append(cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=rng))
    if nsig >= 4:
        cols[1] = np.zeros(A.shape[0])
        cols[2] = A[:, m // 2].astype(np.float64)
        cols[3] = cols[0].copy()
    return np.asfortranarray(np.stack(cols, axis=1))


def check_group_sizes(cs, At, A, k, eps, sizes, seed):
    """for every R in sizes: group_max R and 3R signals (three groups of R; five signals at R = 1), pipelines 3 against 1"""
    d = cs.Dictionary(At)
    gmax = d.ctx.sweep_config()["group_max"]
    for R in sizes:
        assert R <= gmax
        nsig = 3 * R if R > 1 else 5
        B = signals(cs, A, k, nsig, seed + R)
        d.ctx.tune("group_max", 0)
        d.ctx.tune("pipelines", 1)
        ref = d.ctx.omp_batch(B, k, eps)
        d.ctx.tune("group_max", R)
        d.ctx.tune("pipelines", 3)
        got = d.ctx.omp_batch(B, k, eps)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), (R, nsig)
    d.ctx.tune("group_max", 0)
    d.ctx.tune("pipelines", 0)
    d.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [1, 7, 1023, 7921])
def test_shared_sweep_few_and_odd_columns(cs, dtype, N):
    """M = 4096: N below one column pair per wave of the grid, and odd N"""
    M, k = 4096, min(5, N)
    At, A = dictionary(M, N, dtype, 17 + N)
    check_group_sizes(cs, At, A, k, float(np.finfo(dtype).eps), (1, 2, 3, 4), N)


def test_shared_sweep_four_load_units(cs):
    """M = 3000 f32: twelve 256-row chunks (the single body's image runs 4-load units; four images fit)"""
    M, N, k = 3000, 7921, 6
    At, A = dictionary(M, N, np.float32, 5)
    check_group_sizes(cs, At, A, k, float(np.finfo(np.float32).eps), (1, 2, 3, 4), 50)


@pytest.mark.parametrize("N", [7, 1023])
def test_shared_sweep_two_images(cs, N):
    """about 9000 rows f32: two residual images fit beside the scratch"""
    M, k = 9000, 5
    At, A = dictionary(M, N, np.float32, 3 + N)
    check_group_sizes(cs, At, A, k, float(np.finfo(np.float32).eps), (1, 2), 60 + N)
