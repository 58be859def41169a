"""GPU parity tests (pytest -m gpu) of round 17's two changes to csmp_omp_batch's grouped schedule: its shared passes store no c (nothing
reads it there; csmp_tune pass_c 1 stores it as before), and a batch of wide groups ends on a group of four -- a narrow pass -- where
that takes no pass more (csmp_tune group_split 1 keeps the even split).  Neither changes a signal's arithmetic: every setting must give
the bits of one pipeline of single signals (pipelines 1), in the same number of passes, and csmp_mp_batch, whose passes still store
c, must give csmp_mp's bits before and after such a batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, K = 4096, 6
NSIGS = (9, 10, 12, 17, 18, 20, 21, 25)


def close(v, ref, tol=1e-9):
    return np.allclose(v, ref, rtol=tol, atol=tol * (float(np.max(np.abs(ref))) if len(ref) else 0.0))


def groups_of(nsig, R):
    """the (first, size) of the default plan's groups (host/batch_plan.hpp): R = 8, a last group of four where that takes no pass more;
    else, and for R = 4, as even as possible"""
    p = -(-nsig // R)
    if R > 4 and p >= 2 and nsig <= R * (p - 1) + 4:
        rest = nsig - 4
        sizes = [R] * (rest // R) + ([rest % R] if rest % R else []) + [4]
    else:
        sizes = [nsig // p + (1 if i < nsig % p else 0) for i in range(p)]
    return [(sum(sizes[:i]), s) for i, s in enumerate(sizes)]


def dictionary(N, dtype, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(torch.float32 if dtype == np.float32 else torch.float64)
    return At, np.asfortranarray(At.cpu().numpy().T)


def signals(cs, A, nsig, R, seed):
    """planted K-sparse signals plus noise; in the LAST group (the narrow remainder group where the plan has one) a zero signal, one
    atom and a duplicate of signal 0; in the first half of the first group, which is never short of a member, an exactly 2-sparse
    signal: the members of that half stop at different steps.  Returns B and the columns (zero, atom, duplicate, 2-sparse)."""
    rng = np.random.default_rng(seed)
    m = A.shape[1]
    cols = []
    for _ in range(nsig):
        xs = cs.sparse_vector(m, K, rng=rng)
        cols.append(cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=rng))
    first, size = groups_of(nsig, R)[-1]
    assert size >= 3 and first > 1
    cols[first] = np.zeros(A.shape[0])
    cols[first + 1] = A[:, m // 3 + 17].astype(np.float64)
    cols[first + 2] = cols[0].copy()
    xs = cs.sparse_vector(m, 2, rng=rng)
    cols[1] = A[:, xs.nzind].astype(np.float64) @ xs.nzval
    return np.asfortranarray(np.stack(cols, axis=1)), (first, first + 1, first + 2, 1)


def run(d, B, eps, **tunes):
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return d.ctx.omp_batch(B, K, eps)
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


def passes(d, B, eps, **tunes):
    """run(), and the shared passes it launched (every one of them timed: one sampled launch per pass, both pipelines counted)"""
    d.ctx.profile_enable(True)
    d.ctx.profile_read(reset=True)
    out = run(d, B, eps, **tunes)
    n, _ = d.ctx.profile_read(reset=True)
    d.ctx.profile_enable(False)
    return out, n


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def mp_loop(d, B, k):
    """csmp_mp signal by signal, in the batch's output layout: csmp_mp_batch's reference"""
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


@pytest.fixture(scope="module")
def f32(cs):
    At, A = dictionary(3001, np.float32, 17)  # an odd N: the last pair of columns clamps
    d = cs.Dictionary(At)
    yield d, A
    d.close()


def check(cs, oracle, d, A, nsig, eps, with_oracle):
    R = d.ctx.sweep_config()["group_wide"]
    B, (zero, atom, dup, two) = signals(cs, A, nsig, R, 1000 + nsig)
    ref = run(d, B, eps, pipelines=1)
    nnz = ref[2]
    assert nnz[zero] <= 2 and nnz[atom] <= 2 and nnz[two] < K, (nsig, nnz)  # (a zero signal takes one atom: the first sweep checks no eps)
    assert nnz[0] == K and nnz[2] == K and nnz[dup] == K, (nsig, nnz)       # ... beside members that go on
    assert all(np.array_equal(x[..., dup], x[..., 0]) for x in ref)
    got, npass = passes(d, B, eps)
    assert same(ref, got), nsig
    assert npass == K * -(-nsig // R), (nsig, npass)
    for tunes in ({"group_split": 1}, {"pass_c": 1}, {"group_split": 1, "pass_c": 1}):
        got, npass = passes(d, B, eps, **tunes)
        assert same(ref, got), (nsig, tunes)
        assert npass == K * -(-nsig // R), (nsig, tunes, npass)
    if with_oracle:  # a planted signal, the 2-sparse one, and the narrow group's zero signal, atom and duplicate
        idx, val, nnz = run(d, B, eps)
        for s in (0, two, zero, atom, dup):
            want = oracle.omp(A, B[:, s], K, eps)
            assert nnz[s] == len(want[0]) and np.array_equal(idx[:nnz[s], s], want[0]), (nsig, s)
            assert close(val[:nnz[s], s], want[1]), (nsig, s)
    return B


def test_plan_helper():
    assert [s for _, s in groups_of(18, 8)] == [8, 6, 4] and [s for _, s in groups_of(20, 8)] == [8, 8, 4]
    assert [s for _, s in groups_of(9, 8)] == [5, 4] and [s for _, s in groups_of(21, 8)] == [7, 7, 7]
    assert groups_of(25, 8) == [(0, 8), (8, 8), (16, 5), (21, 4)] and [s for _, s in groups_of(18, 4)] == [4, 4, 4, 3, 3]


@pytest.mark.parametrize("nsig", NSIGS)
def test_split_and_pass_c_keep_the_bits(cs, oracle, f32, nsig):
    d, A = f32
    cfg = d.ctx.sweep_config()
    assert cfg["group_max"] == 4 and cfg["group_wide"] == 8
    check(cs, oracle, d, A, nsig, float(np.finfo(np.float32).eps), nsig in (10, 18))


def test_f64_dictionary(cs, oracle):
    """groups of four on the four-wave body (k_sweep_multi_w4): the same predicate, the even split"""
    At, A = dictionary(7920, np.float64, 23)
    d = cs.Dictionary(At)
    cfg = d.ctx.sweep_config()
    assert cfg["group_max"] == 4 and cfg["group_wide"] == 4
    check(cs, oracle, d, A, 18, float(np.finfo(np.float64).eps), False)
    d.close()


def test_mp_batch_passes_still_store_c(cs, oracle, f32):
    """k_mp_group reads c from the slots the grouped OMP passes no longer write: an mp batch before and after an omp batch on the same
    contexts and slots gives csmp_mp's bits"""
    d, A = f32
    eps = float(np.finfo(np.float32).eps)
    B, _ = signals(cs, A, 18, 8, 77)
    want = mp_loop(d, B, 2 * K)
    assert same(want, d.ctx.mp_batch(B, 2 * K))
    omp = run(d, B, eps)
    assert same(want, d.ctx.mp_batch(B, 2 * K))
    assert same(omp, run(d, B, eps, pipelines=1))
