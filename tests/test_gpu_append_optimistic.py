"""GPU tests (pytest -m gpu) of the two ends of a batch round that the grouped scheduler shares among its members.

The append launch (k_append_group) runs optimistic chains only: on a COHERENT dictionary the first Gram-Schmidt pass fails the DGKS
test rho^2 >= |a|^2 / 2 for some members of a group and not for others.  A failing member is flagged by the append kernel, which
commits nothing for it; the flag reaches the host through the round's finish launch, and the member is solved again by the safe
three-kernel chain.  Every batch must equal one csmp_omp call per signal bit for bit, whatever the schedule.
The dictionary is test_omp_coherent_dictionary_triggers_dgks's (A = U S V, spectrum 1 / i^2).  On it nearly every planted signal of k
atoms meets the failing test at some step, so every third member is one that stops after its first atom (a single atom, or a signal
far below eps): its only append is the first column's, rho^2 = |a|^2.  Which member is which is decided on the CPU first, by a Float64
replay of the oracle's selection order.

The finish launch (k_finish_group): one launch per context and round runs the single-wave back substitution and the sorted emission
of every member, each on its own R, z, selection and outputs.  Batches of 1 ... 25 signals, with a zero signal, a one-atom signal
and a duplicate among them, must equal the one-at-a-time calls bit for bit; a support beyond the single-wave form (k = 300) keeps
launch_finish's block back substitution per member and must do the same."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {  # M, N, k, nsig, dtype, tunes of the first run
    "grouped_13": (256, 1024, 8, 13, np.float32, {"pipelines": 3}),
    "wide_4+3": (4096, 3001, 6, 7, np.float32, {}),
    "f64_6": (256, 1024, 8, 6, np.float64, {"pipelines": 3}),
}


def coherent(M, N, dtype, rng):
    U, V = rng.standard_normal((M, M)), rng.standard_normal((M, N))
    A = (U * (1.0 / np.arange(1, M + 1) ** 2)) @ V
    A /= np.linalg.norm(A, axis=0)
    return np.asfortranarray(A.astype(dtype))


def dgks_ratios(A64, order):
    """rho^2 / |a|^2 of the first Gram-Schmidt pass for every column of a selection order, in Float64 (Q from two passes)"""
    Q = np.zeros((A64.shape[0], 0))
    out = []
    for c in order:
        a = A64[:, c]
        w = Q.T @ a
        out.append(float((a @ a - w @ w) / (a @ a)))
        v = a - Q @ w
        v -= Q @ (Q.T @ v)
        Q = np.column_stack([Q, v / np.linalg.norm(v)])
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, B, k, eps, oracle results, flagged members, unflagged members): computed once, shared by the tests, never written to"""
    from csmp_pkg import load
    from oracle import oracle_c
    cs = load()
    oracle_c.build()
    M, N, k, nsig, dtype, _ = SHAPES[name]
    rng = np.random.default_rng(5)
    A = coherent(M, N, dtype, rng)
    A64 = A.astype(np.float64)
    eps = float(np.finfo(dtype).eps)
    cols = []
    for s in range(nsig):
        if s % 3 == 1:  # stops after its first atom: one atom exactly, or (every other one) a planted signal far below eps
            cols.append(A64[:, (N // 3 + 17 * s) % N].copy() if s % 2 else
                        1e-3 * eps * (A64 @ cs.sparse_vector(N, k, rng=rng).to_dense()))
        else:
            cols.append(cs.perturb(A64 @ cs.sparse_vector(N, k, rng=rng).to_dense(), 1e-3, rng=rng))
    B = np.asfortranarray(np.stack(cols, axis=1))
    refs = [oracle_c.omp(A, B[:, s], k, eps) for s in range(nsig)]
    ratios = [dgks_ratios(A64, r[2]) for r in refs]
    flagged = [s for s in range(nsig) if min(ratios[s]) < 0.5]
    unflagged = [s for s in range(nsig) if min(ratios[s]) >= 0.5]
    for a in (A, B):
        a.setflags(write=False)
    return A, B, k, eps, refs, flagged, unflagged, ratios


def run(d, B, k, eps, **tunes):
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    out = d.ctx.omp_batch(B, k, eps)
    for key in tunes:
        d.ctx.tune(key, 0)
    return out


@pytest.fixture(scope="module")
def solved(cs):
    """per shape: the open dictionary and one csmp_omp call per signal"""
    made = {}

    def get(name):
        if name not in made:
            A, B, k, eps = case(name)[:4]
            d = cs.Dictionary(A)
            made[name] = (d, [d.ctx.omp(B[:, s], k, eps) for s in range(B.shape[1])])
        return made[name]
    yield get
    for d, _ in made.values():
        d.close()


def assert_same_bits(got, lone, what):
    idx, val, nnz = got
    for s, (li, lv, _) in enumerate(lone):
        n = int(nnz[s])
        assert n == len(li), (what, s, n, len(li))
        assert np.array_equal(idx[:n, s], li), (what, s)
        assert np.array_equal(val[:n, s].view(np.int64), lv.view(np.int64)), (what, s)


@pytest.mark.parametrize("name", list(SHAPES))
def test_members_that_fail_the_optimistic_chain_beside_members_that_do_not(name, solved):
    A, B, k, eps, refs, flagged, unflagged, ratios = case(name)
    print(name, "min rho^2/|a|^2 per member:", " ".join("%.3f" % min(r) for r in ratios))
    assert len(flagged) >= 1 and len(unflagged) >= 2, (flagged, unflagged)
    d, lone = solved(name)
    got = run(d, B, k, eps, **SHAPES[name][5])
    assert_same_bits(got, lone, name)
    idx, val, nnz = got
    clear = sorted(unflagged, key=lambda s: -min(ratios[s]))[:2]
    for s in flagged + clear:  # the oracle's support: the re-solved members and two the append kernel committed throughout
        assert int(nnz[s]) == len(refs[s][0]) and np.array_equal(idx[:int(nnz[s]), s], refs[s][0]), (name, s, min(ratios[s]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_schedule_gives_the_same_bits(name, solved):
    A, B, k, eps = case(name)[:4]
    d, lone = solved(name)
    base = dict(SHAPES[name][5])
    for tunes in ({"group_wide": 1}, {"group_max": 1}, {"group_max": 2}, {"group_max": 3}):
        assert_same_bits(run(d, B, k, eps, **base, **tunes), lone, (name, tunes))
    for pipes in (1, 2):
        assert_same_bits(run(d, B, k, eps, pipelines=pipes), lone, (name, pipes))


# ---------------------------------------------------------------------------------------------- the finish launch of a round
def incoherent(M, N, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0)
    return np.asfortranarray(A.astype(np.float32))


def finish_signals(cs, A, k, nsig, seed):
    """planted k-sparse signals plus noise; signal 1 a duplicate of signal 0, signal 2 zero, signal 3 one atom exactly (as far as
    there are that many)"""
    rng = np.random.default_rng(seed)
    A64 = A.astype(np.float64)
    cols = [cs.perturb(A64 @ cs.sparse_vector(A.shape[1], k, rng=rng).to_dense(), 5e-3, rng=rng) for _ in range(nsig)]
    if nsig > 1:
        cols[1] = cols[0].copy()
    if nsig > 2:
        cols[2] = np.zeros(A.shape[0])
    if nsig > 3:
        cols[3] = A64[:, A.shape[1] // 3].copy()
    return np.asfortranarray(np.stack(cols, axis=1))


@pytest.fixture(scope="module")
def small(cs):
    d = cs.Dictionary(incoherent(256, 1024, 21))
    yield d
    d.close()


@pytest.mark.parametrize("nsig", [1, 2, 5, 13, 18, 25])
def test_one_finish_launch_per_round_gives_the_bits_of_single_calls(cs, small, nsig):
    k, eps = 5, float(np.finfo(np.float32).eps)
    A = incoherent(256, 1024, 21)
    B = finish_signals(cs, A, k, nsig, 100 + nsig)
    lone = [small.ctx.omp(B[:, s], k, eps) for s in range(nsig)]
    got = run(small, B, k, eps, pipelines=3)
    assert_same_bits(got, lone, nsig)
    idx, val, nnz = got
    for s in range(nsig):  # past a member's count: launch_finish's fill
        assert np.all(idx[int(nnz[s]):, s] == -1) and np.all(val[int(nnz[s]):, s] == 0.0), s
    if nsig > 3:
        assert int(nnz[2]) <= 1 and int(nnz[3]) == 1 and idx[0, 3] == 1024 // 3
        assert all(int(nnz[s]) == k for s in (0, 1, 4))
    for pipes in (1, 2):  # the tick pipelines end their rounds with the same launch
        assert_same_bits(run(small, B, k, eps, pipelines=pipes), lone, (nsig, pipes))


def test_supports_beyond_the_single_wave_keep_their_own_finish(cs):
    """k = 300: kcap > 256, launch_finish's super-blocks (k_trsv_*), one member at a time as before"""
    M, N, k, nsig = 512, 2048, 300, 5
    eps = float(np.finfo(np.float32).eps)
    A = incoherent(M, N, 22)
    B = finish_signals(cs, A, 40, nsig, 7)
    d = cs.Dictionary(A)
    try:
        lone = [d.ctx.omp(B[:, s], k, eps) for s in range(nsig)]
        assert max(len(li) for li, _, _ in lone) > 256
        assert_same_bits(run(d, B, k, eps, pipelines=3), lone, "k300")
    finally:
        d.close()
