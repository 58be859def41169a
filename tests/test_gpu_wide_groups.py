"""GPU parity tests (pytest -m gpu) of the wide groups of csmp_omp_batch's grouped scheduler: a pass over a Float32 dictionary serves
up to eight signals as two halves of up to four, on two workgroups that read the same bytes of A (k_sweep_wide).  Every signal keeps
its own arithmetic, so the runs with wide groups must give the bits of one pipeline of single signals (pipelines 1): supports,
coefficients and counts -- with halves of equal and unequal size, a remainder group of four or fewer, an odd N, a half whose members
have all stopped beside one that goes on, group_wide 1 (off), a tick grid that is no multiple of 16, a Float64 dictionary (which
keeps groups of four), and a device that cannot hold the 24 slots (groups of four then)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSIGS = (5, 6, 7, 8, 9, 13, 18, 20, 25)


def close(v, ref, tol=1e-9):
    return np.allclose(v, ref, rtol=tol, atol=tol * (float(np.max(np.abs(ref))) if len(ref) else 0.0))


def dictionary(M, N, dtype, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(torch.float32 if dtype == np.float32 else torch.float64)
    return At, np.asfortranarray(At.cpu().numpy().T)


def halves(nsig, members=8):
    """the (first, size) of the second half of every wide group of the plan: groups of consecutive signals, as even as possible"""
    ngroups = (nsig + members - 1) // members
    out, at = [], 0
    for i in range(ngroups):
        size = nsig // ngroups + (1 if i < nsig % ngroups else 0)
        if size > 4:
            out.append((at + (size + 1) // 2, size // 2))
        at += size
    return out


def signals(cs, A, k, nsig, seed):
    """planted k-sparse signals plus noise.  The SECOND half of the first wide group holds only signals that stop at once or after one
    or two steps -- a zero signal, one atom, an exactly 2-sparse signal, then more single atoms -- while its first half goes on; signal 1
    is a duplicate of signal 0."""
    rng = np.random.default_rng(seed)
    m = A.shape[1]
    cols = []
    for _ in range(nsig):
        xs = cs.sparse_vector(m, k, rng=rng)
        cols.append(cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=rng))
    hs = halves(nsig)
    if hs:
        first, size = hs[0]
        for j in range(size):
            if j == 0:
                cols[first] = np.zeros(A.shape[0])
            elif j == 2:
                xs = cs.sparse_vector(m, 2, rng=rng)
                cols[first + j] = A[:, xs.nzind].astype(np.float64) @ xs.nzval
            else:
                cols[first + j] = A[:, (m // 3 + 17 * j) % m].astype(np.float64)
    cols[1] = cols[0].copy()
    return np.asfortranarray(np.stack(cols, axis=1))


def run(d, B, k, eps, **tunes):
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    out = d.ctx.omp_batch(B, k, eps)
    for key in tunes:
        d.ctx.tune(key, 0)
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def passes(d, B, k, eps, **tunes):
    """run(), and the shared passes it launched (every one of them timed: one sampled launch per pass, both pipelines counted)"""
    d.ctx.profile_enable(True)
    d.ctx.profile_read(reset=True)
    out = run(d, B, k, eps, **tunes)
    n, _ = d.ctx.profile_read(reset=True)
    d.ctx.profile_enable(False)
    return out, n


def test_plan_halves_helper():
    assert halves(6) == [(3, 3)] and halves(7) == [(4, 3)] and halves(4) == [] and halves(9) == [(3, 2)]
    assert halves(18) == [(3, 3), (9, 3), (15, 3)] and halves(20) == [(4, 3), (11, 3), (17, 3)]


@pytest.mark.parametrize("N,nsigs", [(65536, (18, 7)), (7920, NSIGS), (3001, NSIGS)])
def test_wide_groups_give_the_bits_of_one_pipeline(cs, oracle, N, nsigs):
    M, k = 4096, 6
    eps = float(np.finfo(np.float32).eps)
    At, A = dictionary(M, N, np.float32, 11 + N)
    d = cs.Dictionary(At)
    cfg = d.ctx.sweep_config()
    assert cfg["group_max"] == 4 and cfg["group_wide"] == 8
    for nsig in nsigs:
        B = signals(cs, A, k, nsig, nsig + N)
        ref = run(d, B, k, eps, pipelines=1)
        wide, npass = passes(d, B, k, eps)
        assert same(ref, wide), nsig
        # the wide groups were really taken: k passes for every group of up to EIGHT signals (a stopped group's pass is still launched)
        assert npass == k * ((nsig + 7) // 8), (nsig, npass)
        narrow, npass = passes(d, B, k, eps, group_wide=1)
        assert same(ref, narrow) and npass == k * ((nsig + 3) // 4), (nsig, npass)
        first, size = halves(nsig)[0]
        assert all(ref[2][first + j] <= 2 for j in range(size)), nsig  # the half that stops (a zero signal takes one atom: the first sweep checks no eps) ...
        assert all(ref[2][s] == k for s in range(first)), nsig  # ... beside the one that goes on
        assert same(ref, run(d, B, k, eps, pipelines=3)), nsig
        assert same(ref, run(d, B, k, eps, group_wide=1)), nsig
        if nsig in (7, 18) and N != 3001:  # against the oracle: a planted signal, the stopped ones, the duplicate
            idx, val, nnz = wide
            for s in (0, 1, first, first + 1, first + 2):
                want = oracle.omp(A, B[:, s], k, eps)
                assert nnz[s] == len(want[0]) and np.array_equal(idx[:nnz[s], s], want[0]), (nsig, s)
                assert close(val[:nnz[s], s], want[1]), (nsig, s)
    d.close()


def test_group_wide_switch_and_tick_grid(cs):
    M, N, k = 4096, 7920, 5
    eps = float(np.finfo(np.float32).eps)
    At, A = dictionary(M, N, np.float32, 5)
    d = cs.Dictionary(At)
    B = signals(cs, A, k, 13, 99)
    ref = run(d, B, k, eps, pipelines=1)
    d.ctx.tune("group_wide", 1)
    cfg = d.ctx.sweep_config()
    assert cfg["group_max"] == 4 and cfg["group_wide"] == 4
    assert same(ref, d.ctx.omp_batch(B, k, eps))
    d.ctx.tune("group_wide", 0)
    assert d.ctx.sweep_config()["group_wide"] == 8
    for gm in (1, 2, 3, 4):  # an explicit group_max: the narrow groups only
        d.ctx.tune("group_max", gm)
        cfg = d.ctx.sweep_config()
        assert cfg["group_max"] == gm and cfg["group_wide"] == gm
    d.ctx.tune("group_max", 0)
    for grid in (200, 203, 17, 16, 7, 96, 400):  # the wide grid is rounded down to a multiple of 16 (at least 16)
        assert same(ref, run(d, B, k, eps, tick_grid=grid)), grid
    d.close()


def test_f64_dictionary_keeps_groups_of_four(cs):
    M, N, k = 4096, 3001, 5
    eps = float(np.finfo(np.float64).eps)
    At, A = dictionary(M, N, np.float64, 6)
    d = cs.Dictionary(At)
    cfg = d.ctx.sweep_config()
    assert cfg["group_max"] == 4 and cfg["group_wide"] == 4
    for nsig in (6, 13):
        B = signals(cs, A, k, nsig, 7 + nsig)
        ref = run(d, B, k, eps, pipelines=1)
        assert same(ref, run(d, B, k, eps)), nsig
        assert same(ref, run(d, B, k, eps, group_wide=1)), nsig
    d.close()


def test_without_the_wide_slots_groups_of_four(cs):
    """The slots beyond the narrow groups' are all there or none: every allocation of theirs, on either context, made to fail in turn
    (fail_alloc) leaves a batch that runs groups of four and returns the same bits -- and the next batch, with nothing failing, too."""
    M, N, k, nsig = 256, 1024, 4, 13
    eps = float(np.finfo(np.float32).eps)
    At, A = dictionary(M, N, np.float32, 8)
    B = signals(cs, A, k, nsig, 3)
    d = cs.Dictionary(At)
    d.ctx.tune("pipelines", 3)  # (a small dictionary: the grouped scheduler on request)
    assert d.ctx.sweep_config()["group_wide"] == 8
    d.ctx.tune("group_wide", 1)
    ref = d.ctx.omp_batch(B, k, eps)  # the narrow slots of both contexts exist from here on
    d.ctx.tune("group_wide", 0)
    from csmp_pkg import load
    L = load()._lib
    blocks = L.live_resources()["device_blocks"]
    # what the wide slots of both contexts take, counted on a second dictionary: the blocks one wide batch adds to a narrow one's
    d2 = cs.Dictionary(At)
    d2.ctx.tune("pipelines", 3)
    d2.ctx.tune("group_wide", 1)
    d2.ctx.omp_batch(B, k, eps)
    b2 = L.live_resources()["device_blocks"]
    d2.ctx.tune("group_wide", 0)
    assert same(ref, d2.ctx.omp_batch(B, k, eps))
    wide_allocs = L.live_resources()["device_blocks"] - b2
    d2.close()
    assert wide_allocs >= 2 * 12 * 30 and L.live_resources()["device_blocks"] == blocks, wide_allocs  # (twelve more slots on each context)
    # the call's own staging buffers come first, and a failure of theirs fails the call, as it always has
    staged = 0
    while True:
        d.ctx.tune("fail_alloc", staged + 1)
        try:
            got = d.ctx.omp_batch(B, k, eps)
            break
        except cs.CsmpError as e:
            assert e.code in (L.EHIP, L.ENOMEM) and staged < 16, (staged, e.code, str(e))
            staged += 1
        finally:
            d.ctx.tune("fail_alloc", 0)
    # then EVERY allocation of the wide slots in turn: the batch goes through on the slots it had, and none of the wide ones stays
    for n in range(staged + 1, staged + wide_allocs + 1):
        d.ctx.tune("fail_alloc", n)
        got = d.ctx.omp_batch(B, k, eps)
        d.ctx.tune("fail_alloc", 0)
        assert same(ref, got), n
        assert L.live_resources()["device_blocks"] == blocks, n
    for _ in range(2):  # with nothing failing: the wide slots are allocated, then reused
        assert same(ref, d.ctx.omp_batch(B, k, eps))
        assert L.live_resources()["device_blocks"] == blocks + wide_allocs
    d.close()
