"""GPU parity tests (pytest -m gpu): the HIP path, called through the C ABI (libcsmp.so via the
ctypes host mirror), against the CPU oracle on the same seeded inputs and against the committed
golden vectors.  Bar: identical supports / selection order (integer work: bit-exact), coefficients
within 1e-6 relative in Float64 (north_star) -- in practice ~1e-13."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RTOL = 1e-6  # BASELINE.json north_star: "coefficients within 1e-6 relative Float64"
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


def _usable_cores():
    """min(affinity, cgroup quota): the GPU boxes show 256 logical CPUs under a 16-CPU quota, and an OpenMP team of 256 makes the
    oracle's sweeps several times slower."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:  # noqa: BLE001
        pass
    return n


NT = _usable_cores()  # OpenMP threads for the oracle's full-size solves
DEFAULT_SCREEN = 3  # CSMP_OPT_BATCH_SCREEN's default: binary16 operands (include/csmp.h)


def close(v, ref, tight=True):
    tol = 1e-9 if tight else RTOL
    return np.allclose(v, ref, rtol=tol, atol=tol * max(1e-300, float(np.max(np.abs(ref))) if len(ref) else 0.0))


@pytest.fixture
def D(cs):
    """dictionaries of ONE test, closed when it ends (a module-wide list kept some three hundred contexts -- each with its stream, and
    since round 6 a twin context with another -- alive at once for no reason)"""
    made = []

    def make(A):
        d = cs.Dictionary(A)
        made.append(d)
        return d
    yield make
    for d in made:
        d.close()


def test_library_is_the_hip_one(cs):
    d = cs.Context(0)
    name, cus, mem = d.device_info()
    assert "gfx950" in name and cus >= 200, name
    d.close()


def test_golden_vectors_through_the_abi(cs, golden, D):
    ran = 0
    for name, c in golden.items():
        A, b, p = c["A"], c["b"], c["params"]
        d = D(A)
        if c["algo"] == "omp":
            idx, val, order = d.ctx.omp(b, int(p[0]), float(p[1]))
            assert np.array_equal(order, c["order"]), name
        elif c["algo"] == "mp":
            idx, val = d.ctx.mp(b, int(p[0]))
        elif c["algo"] == "gomp":
            idx, val, order = d.ctx.gomp(b, int(p[0]), int(p[1]), float(p[2]))
            assert np.array_equal(order, c["order"]), (name, order, c["order"])
        elif c["algo"] in ("br", "lace"):
            idx, val = d.ctx.br(b, float(p[0]), float(p[1]), int(p[2]), lace=c["algo"] == "lace")
        elif c["algo"] == "rmp_k":
            idx, val = d.ctx.rmp(b, int(p[0]))
        elif c["algo"] == "rmp_delta":
            idx, val = d.ctx.rmp(b, float(p[0]), int(p[1]))
        elif c["algo"] == "foba":
            idx, val = d.ctx.foba(b, float(p[0]))
        elif c["algo"] == "srr":
            idx, val, iters = d.ctx.srr(b, int(p[0]), float(p[1]), -1, int(p[2]), int(p[3]))
            assert iters == int(p[4]), name
        elif c["algo"] == "fr":
            idx, val, order = d.ctx.fr(b, int(p[0]), float(p[1]), float(p[2]))
            assert np.array_equal(order, c["order"]), (name, order, c["order"])
        elif c["algo"] == "ompr":
            idx, val, iters = d.ctx.ompr(b, int(p[0]), float(p[1]))
            assert iters == int(p[2]), name
        elif c["algo"] in ("sp_steps", "ompr_steps"):  # the step-level functors: acquisition + `steps` update! calls
            P = (cs.SP if c["algo"] == "sp_steps" else cs.OMPR)(d, b, int(p[0]))
            xv = cs.sp_acquisition(P) if c["algo"] == "sp_steps" else cs.oblivious_acquisition(P, None, int(p[0]))
            for _ in range(int(p[1])):
                xv = P(xv)
            idx, val = xv.nzind, xv.nzval
            P.close()
        else:
            idx, val, iters = d.ctx.sp(b, int(p[0]), float(p[1]))
            assert iters == int(p[2]), name
        assert np.array_equal(idx, c["idx"]), (name, idx, c["idx"])
        if np.all(np.isfinite(c["val"])):
            assert close(val, c["val"]), (name, val, c["val"])
        else:  # gomp_dupcols: an atom AND its exact copy are both selected -> singular least squares;
            pass  # the reference's own coefficients are NaN/Inf there, only the support is defined
        ran += 1
    assert ran == len(golden) >= 44


@pytest.mark.parametrize("shape", [(32, 48, 3), (64, 256, 8), (37, 101, 5), (256, 1024, 32), (130, 700, 20), (512, 4096, 40)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_omp_matches_oracle(cs, oracle, D, shape, dtype):
    n, m, k = shape
    eps = float(np.finfo(dtype).eps)
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n * 31 + m, dtype=dtype)
    d = D(A)
    for seed in range(3):
        xs = cs.sparse_vector(m, k, rng=seed)
        y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=seed + 100)
        ref = oracle.omp(A, y, k, eps)
        got = d.ctx.omp(y, k, eps)
        assert np.array_equal(got[2], ref[2]), "selection order"
        assert np.array_equal(got[0], ref[0])
        assert close(got[1], ref[1])
        # the public driver, same defaults as the reference: omp(A, b, k)
        xv = cs.omp(d, y, k)
        assert np.array_equal(xv.nzind, ref[0]) and close(xv.nzval, ref[1])


def test_omp_coherent_dictionary_triggers_dgks(cs, oracle, D):
    """correlated_data (src/util.jl:34-47): A = U S V with a 1/i^2 spectrum -- atoms are highly
    coherent, the first Gram-Schmidt pass cancels and the re-orthogonalisation must kick in.
    Coefficients are compared at the north_star tolerance scaled by the conditioning."""
    rng = np.random.default_rng(5)
    n, m, k = 64, 200, 6
    U, V = rng.standard_normal((n, n)), rng.standard_normal((n, m))
    A = (U * (1.0 / np.arange(1, n + 1) ** 2)) @ V
    A /= np.linalg.norm(A, axis=0)
    A = np.asfortranarray(A)
    xs = cs.sparse_vector(m, k, rng=rng)
    y = cs.perturb(A @ xs.to_dense(), 1e-3, rng=rng)
    d = D(A)
    ref = oracle.omp(A, y, k, EPS64)
    got = d.ctx.omp(y, k, EPS64)
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0])
    cond = np.linalg.cond(A[:, ref[0]])
    assert np.allclose(got[1], ref[1], rtol=1e-6, atol=1e-12 * cond * np.abs(ref[1]).max()), (cond, got[1], ref[1])
    # the batch driver runs the optimistic two-kernel chain first, sees the device flag and repeats
    # the flagged signals with the second Gram-Schmidt pass: same answers
    B = np.asfortranarray(np.stack([y, cs.perturb(A @ cs.sparse_vector(m, k, rng=rng).to_dense(), 1e-3, rng=rng), y], axis=1))
    idx, val, nnz = d.ctx.omp_batch(B, k, EPS64)
    for s_ in range(3):
        r_ = oracle.omp(A, B[:, s_], k, EPS64)
        assert nnz[s_] == len(r_[0]) and np.array_equal(idx[:nnz[s_], s_], r_[0])
        assert np.allclose(val[:nnz[s_], s_], r_[1], rtol=1e-6, atol=1e-10)


def test_omp_b_dtype_f32(cs, oracle, D):
    A, x, b = cs.sparse_data(n=64, m=256, k=6, rng=3, dtype=np.float32)
    y = cs.perturb(b, 5e-3, rng=4).astype(np.float32)
    d = D(A)
    ref = oracle.omp(A, y.astype(np.float64), 6, EPS32)
    got = d.ctx.omp(y, 6, EPS32)
    assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])


def test_omp_keyword_and_eps_forms(cs, oracle, D):
    A, x, b = cs.sparse_data(n=48, m=128, k=3, rng=51)
    d = D(A)
    ref = oracle.omp(A, b, 10, 1e-8)
    for xv in (cs.omp(d, b, 1e-8, 10), cs.omp(d, b, max_residual=1e-8, sparsity=10)):
        assert np.array_equal(xv.nzind, ref[0]) and close(xv.nzval, ref[1])
    assert len(ref[0]) == 3  # eps-stop after the planted atoms
    xv = cs.omp(d, b, 1e-8)  # k defaults to size(A,1)
    assert np.array_equal(xv.nzind, ref[0])
    with pytest.raises(ValueError):
        cs.omp(d, b, -1.0, 3)
    with pytest.raises(cs.CsmpError):  # the ABI itself refuses too (CSMP_EINVAL)
        d.ctx.omp(b, 3, -1.0)
    with pytest.raises(cs.CsmpError):  # CSMP_EDIM
        d.ctx.omp(b[:-1], 3, 0.0)


@pytest.mark.parametrize("shape", [(32, 48, 3, 2), (64, 256, 9, 4), (37, 101, 7, 3), (256, 1024, 32, 4), (300, 5000, 40, 16), (128, 3000, 60, 20)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gomp_matches_oracle(cs, oracle, D, shape, dtype):
    n, m, k, l = shape
    eps = float(np.finfo(dtype).eps)
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n * 17 + m, dtype=dtype)
    d = D(A)
    for seed in range(2):
        xs = cs.sparse_vector(m, k, rng=seed)
        y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=seed + 50)
        ref = oracle.gomp(A, y, l, k, eps)
        got = d.ctx.gomp(y, l, k, eps)
        assert np.array_equal(got[2], ref[2]), "insertion order"
        assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
        xv = cs.gomp(d, y, l, k)
        assert np.array_equal(xv.nzind, ref[0]) and close(xv.nzval, ref[1])


@pytest.mark.parametrize("shape", [(32, 64, 3), (64, 256, 8), (50, 301, 5), (256, 1024, 24), (512, 8192, 40)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sp_matches_oracle(cs, oracle, D, shape, dtype):
    n, m, k = shape
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n * 13 + m, dtype=dtype)
    d = D(A)
    for seed, delta in ((0, 1e-12), (1, 1e-2)):
        xs = cs.sparse_vector(m, k, rng=seed)
        y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=seed + 60)
        ref = oracle.sp(A, y, k, delta)
        got = d.ctx.sp(y, k, delta)
        assert got[2] == ref[2], "number of update! calls"
        assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
    xv = cs.sp(d, y, k, 1e-2)
    assert np.array_equal(xv.nzind, ref[0])
    with pytest.raises(ValueError):
        cs.sp(d, y, n // 2 + 1)
    with pytest.raises(cs.CsmpError):
        d.ctx.sp(y, n // 2 + 1, 1e-12)  # CSMP_ERANGE from the ABI itself


def test_sp_whole_set_path_and_gram_reuse(cs, oracle, D):
    """Supports of >= 64 atoms go through the whole-set least squares (Gram + blocked Cholesky, csrc/csmp_gram.hpp), and the second
    solve of an SP iteration (the k atoms kept out of the 2k) gathers its Gram matrix from the first one's.  Noisy data, several
    iterations, against the oracle (the append-chain form of the same least squares is what every support below 64 atoms and
    every coherent set takes: test_sp_matches_oracle, test_omp_coherent_dictionary_triggers_dgks)."""
    n, m, k = 640, 4096, 96
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=77, dtype=np.float32)
    d = D(A)
    for seed, noise in ((0, 5e-3), (1, 1e-1), (2, 3e-1)):
        xs = cs.sparse_vector(m, k + 8, rng=seed)
        y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, noise, rng=seed + 9)
        ref = oracle.sp(A, y, k, 1e-12)
        got = d.ctx.sp(y, k, 1e-12)
        assert got[2] == ref[2], "number of update! calls"
        assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
        again = d.ctx.sp(y, k, 1e-12)  # (a second solve starts from a context that holds the first one's kept Gram matrix)
        assert np.array_equal(got[0], again[0]) and got[2] == again[2] and np.array_equal(got[1], again[1])


def test_topk_sweep_semantics(cs, oracle, D):
    """argmaxinner!(P, k): descending by |<a,r>|, ties by ascending index -- both selection paths
    (arg-max rounds for small k, radix select for large k), including exact ties and r = 0."""
    rng = np.random.default_rng(11)
    A = rng.standard_normal((96, 5000)).astype(np.float32)
    A[:, 4000] = A[:, 7]
    A[:, 123] = A[:, 7]
    A = np.asfortranarray(A)
    d = D(A)
    r = rng.standard_normal(96) + 2.0 * A[:, 7]
    ref_abs, _ = oracle.sweep_abs(A, r)
    for k in (1, 2, 5, 16, 17, 40, 96):
        out, ti, tv = d.ctx.sweep(r, k)
        ref = oracle.topk_desc(ref_abs if k > 1 else out, k)
        want = oracle.topk_desc(out, k)  # the device's own |c| values define the order exactly
        assert np.array_equal(ti, want), (k, ti, want)
        assert np.array_equal(np.sort(ti), np.sort(ref)) or k > 1
        np.testing.assert_array_equal(tv, out[ti])
    out, ti, tv = d.ctx.sweep(np.zeros(96), 40)  # every |c| ties at 0: the 40 lowest indices
    assert np.array_equal(ti, np.arange(40))
    assert np.array_equal(cs.argmaxinner(d, r, 5), oracle.topk_desc(d.ctx.sweep(r, 1)[0], 5))


def test_topk_radix_select_buckets_and_ties(cs, oracle, D):
    """The radix select (large k) on data built to stress its bucket logic: |c| taken from a few exact levels (every bucket is
    one massive tie: more ties than the bucket list holds -> in-order scan; fewer -> ranked by index), values that share their
    leading 22 bits (the selection does not settle after two passes), and plain Gaussian data of reference size."""
    rng = np.random.default_rng(3)

    def check(levels, ks):
        n = levels.size
        A = np.zeros((1024, n), np.float32, order="F")  # (k <= size(A,1) is the ABI's bound)
        A[0] = levels
        d = D(A)
        r = np.zeros(1024)
        r[0] = 1.0
        for k in ks:
            out, ti, tv = d.ctx.sweep(r, k)
            np.testing.assert_array_equal(out, np.abs(levels.astype(np.float64)))
            want = oracle.topk_desc(out, k)
            assert np.array_equal(ti, want), (k, ti[:8], want[:8])
            np.testing.assert_array_equal(tv, out[ti])

    # 3 levels, 20000 atoms: the bucket of the k-th key is a tie of ~6700 (> 4096 kept) or, for k small, the top level
    check(rng.choice(np.array([0.25, 0.5, 1.0], np.float32), 20000) * rng.choice(np.array([-1, 1], np.float32), 20000), (40, 300, 1000))
    # 60 levels, 6000 atoms: ties of ~100 inside the bucket
    check(rng.choice(np.linspace(0.1, 0.9, 60).astype(np.float32), 6000), (33, 500, 1023))
    # distinct values that agree in sign, exponent and 11 leading mantissa bits: 1 + j * 2^-20, j < 9000
    check((1.0 + np.arange(9000) * 2.0 ** -20).astype(np.float32)[rng.permutation(9000)], (64, 700))
    # Gaussian, N = 131072 (configs[4]'s N), k = 512 and 1023
    check(rng.standard_normal(131072).astype(np.float32), (512, 1023))


def test_lstsq_pin(cs, oracle, D):
    # test/forward.jl:23-28: "P.AiQR \\ y ~ A[:, nzind] \\ y" -- the reference's one direct pin of the QR
    A, x, b = cs.sparse_data(n=32, m=48, k=3, rng=5)
    y = cs.perturb(b, 1e-2, rng=6)
    d = D(A)
    np.testing.assert_allclose(d.ctx.lstsq([0, 1, 2], y), np.linalg.lstsq(A[:, [0, 1, 2]], y, rcond=None)[0], rtol=1e-10)
    A, x, b = cs.sparse_data(n=200, m=400, k=3, rng=7, dtype=np.float32)
    cols = np.array([399, 5, 60, 3, 17, 40, 41, 2, 250, 251])
    got = d2 = None
    d2 = D(A)
    got = d2.ctx.lstsq(cols, b)
    np.testing.assert_allclose(got, np.linalg.lstsq(A[:, cols].astype(np.float64), b, rcond=None)[0], rtol=1e-9, atol=1e-12)
    with pytest.raises(cs.CsmpError):
        d2.ctx.lstsq([1, 1], b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lstsq_sizes_across_the_solver_paths(cs, oracle, D, dtype):
    """csmp_lstsq = factorize! + ldiv! (src/matchingpursuit.jl:219-227) at the sizes where the implementation changes gear: the
    append chain (< 64 columns), the whole-set path (Gram + blocked Cholesky: 64 and up; bordered column at the start / inside / at
    the end of a 32-block), the single-wave back substitution (<= 256) and the super-block one (> 256: one, two, four super-blocks,
    full and partial), up to the 1023-column capacity -- against numpy's least squares on the promoted matrix."""
    rng = np.random.default_rng(21)
    M, N = 1200, 1500
    A = np.asfortranarray(rng.standard_normal((M, N)).astype(dtype))
    d = D(A)
    b = rng.standard_normal(M)
    for n in (1, 7, 63, 64, 65, 95, 96, 97, 128, 255, 256, 257, 300, 511, 512, 513, 768, 1000, 1023):
        cols = rng.permutation(N)[:n]
        got = d.ctx.lstsq(cols, b)
        want = np.linalg.lstsq(A[:, cols].astype(np.float64), b, rcond=None)[0]
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-11, err_msg=f"n = {n}")


def test_step_level_gomp_functor(cs, oracle, D):
    A, x, b = cs.sparse_data(n=64, m=256, k=6, rng=14)
    y = cs.perturb(b, 5e-3, rng=15)
    d = D(A)
    P = cs.GOMP(d, y, 2)
    xv = cs.spzeros(256)
    for t in range(3):
        cs.update_(P, xv)
        assert xv.nnz == 2 * (t + 1)
        assert close(xv.nzval, oracle.lstsq_cols(A, xv.nzind, y))
    ref = oracle.gomp(A, y, 2, 6, 0.0)
    assert np.array_equal(xv.nzind, ref[0]) and close(xv.nzval, ref[1])


def test_mp_matches_oracle(cs, oracle, D):
    for (n, m, k, dtype) in [(32, 48, 30, np.float64), (64, 256, 50, np.float32), (37, 101, 25, np.float32)]:
        A, x, b = cs.sparse_data(n=n, m=m, k=3, rng=n + m, dtype=dtype)
        # noisy b: the residual stays far above round-off for all k steps.  (On noiseless data MP
        # converges to ||r|| ~ 1e-16 and later picks are decided by rounding noise -- there the
        # incremental device residual and the reference's from-scratch one legitimately differ.)
        b = cs.perturb(b, 5e-2, rng=1)
        d = D(A)
        ref = oracle.mp(A, b, k)
        got = d.ctx.mp(b, k)
        assert np.array_equal(got[0], ref[0])
        assert close(got[1], ref[1])
        # warm start: mp(A,b,k2,x) continues from x (src/matchingpursuit.jl:34)
        x1 = cs.mp(d, b, 7)
        x2 = cs.mp(d, b, k - 7, x1)
        assert np.array_equal(x2.nzind, ref[0]) and close(x2.nzval, ref[1])


def test_sweep_primitive(cs, oracle, D):
    rng = np.random.default_rng(0)
    for (n, m, dtype) in [(32, 48, np.float64), (256, 1024, np.float32), (37, 101, np.float32), (1024, 5000, np.float32), (129, 333, np.float64)]:
        A = np.asfortranarray(rng.standard_normal((n, m)).astype(dtype))
        r = rng.standard_normal(n)
        d = D(A)
        out, ti, tv = d.ctx.sweep(r, 1)
        ref, best = oracle.sweep_abs(A, r)
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-13)
        assert int(ti[0]) == best
        assert cs.argmaxinner(d, r) == best


def test_duplicate_columns_tie_goes_to_lowest_index(cs, D):
    rng = np.random.default_rng(5)
    A = rng.standard_normal((64, 300)).astype(np.float32)
    A[:, 250] = A[:, 17]
    A[:, 299] = A[:, 17]
    A = np.asfortranarray(A)
    r = A[:, 17].astype(np.float64) * 3.0  # makes atom 17 (and its copies) the arg-max
    d = D(A)
    out, ti, tv = d.ctx.sweep(r, 1)
    assert out[17] == out[250] == out[299] and int(ti[0]) == 17


def test_omp_batch_equals_single_signal_calls(cs, oracle, D):
    A, x, b = cs.sparse_data(n=64, m=256, k=5, rng=8, dtype=np.float32)
    d = D(A)
    rng = np.random.default_rng(9)
    B = np.asfortranarray(np.stack([cs.perturb(A.astype(np.float64) @ cs.sparse_vector(256, 5, rng=rng).to_dense(), 5e-3, rng=rng) for _ in range(6)], axis=1))
    xs = cs.omp_batch(d, B, 5)
    for s, xv in enumerate(xs):
        ref = oracle.omp(A, B[:, s], 5, EPS32)
        assert np.array_equal(xv.nzind, ref[0]) and close(xv.nzval, ref[1])
    # float32 signals, device-resident in/out (the bench path)
    import torch
    Bt = torch.from_numpy(np.ascontiguousarray(B.T.astype(np.float32))).cuda()
    idx = torch.empty((6, 5), dtype=torch.int64, device="cuda")
    val = torch.empty((6, 5), dtype=torch.float64, device="cuda")
    nnz = torch.empty(6, dtype=torch.int64, device="cuda")
    d.ctx.omp_batch_device(Bt, 5, EPS32, idx, val, nnz)
    d.ctx.sync()
    for s in range(6):
        ref = oracle.omp(A, B[:, s].astype(np.float32).astype(np.float64), 5, EPS32)
        n = int(nnz[s])
        assert np.array_equal(idx[s, :n].cpu().numpy(), ref[0]) and close(val[s, :n].cpu().numpy(), ref[1])


def test_step_level_omp_functor(cs, oracle, D):
    A, x, b = cs.sparse_data(n=64, m=256, k=6, rng=12)
    y = cs.perturb(b, 5e-3, rng=13)
    d = D(A)
    P = cs.OMP(d, y, 6)
    xv = cs.spzeros(256)
    ref = oracle.omp(A, y, 6, 0.0)
    for t in range(6):
        P(xv)  # (U::Update)(x) = update!(U, x)
        assert xv.nnz == t + 1 and np.array_equal(np.sort(ref[2][:t + 1]), xv.nzind)
        step_ref = oracle.lstsq_cols(A, xv.nzind, y)  # update! leaves x = LS solution on the support
        assert close(xv.nzval, step_ref)
        rn = np.linalg.norm(oracle.residual(A, xv.nzind, xv.nzval, y))
        assert abs(P.resnorm - rn) <= 1e-9 * max(rn, 1e-30)
    assert np.array_equal(xv.nzind, ref[0]) and close(xv.nzval, ref[1])


def test_device_dictionary_is_borrowed_zero_copy(cs, oracle):
    import torch
    A, x, b = cs.sparse_data(n=64, m=256, k=5, rng=20, dtype=np.float32)
    y = cs.perturb(b, 5e-3, rng=21)
    At = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()  # (N, M): row j = atom j
    d = cs.Dictionary(At)
    ref = oracle.omp(A, y, 5, EPS32)
    xv = cs.omp(d, y, 5)
    assert np.array_equal(xv.nzind, ref[0]) and close(xv.nzval, ref[1])
    d.close()


def test_full_size_config2_properties(cs, oracle):
    """BASELINE configs[1] at its real size (4096 x 65536 f32, k = 256): the FULL trajectory of three signals against the
    oracle -- selection order, support, coefficients to 1e-6 -- through csmp_omp (one call at a time) and through csmp_omp_batch
    (the pipelined k_tick path the bench times); then size-independent properties of the full solve (distinct sorted support,
    LS optimality on it, bit-identical re-run, planted recovery) and sweep linearity."""
    import torch
    M, N, k = 4096, 65536, 256
    g = torch.Generator(device="cuda").manual_seed(1234)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float32)
    At /= At.norm(dim=1, keepdim=True)
    d = cs.Dictionary(At)
    A = np.asfortranarray(At.cpu().numpy().T)
    sigs, planted, refs = [], [], []
    for s_ in range(3):
        xs = cs.sparse_vector(N, k, rng=1 + 10 * s_)
        planted.append(xs)
        sigs.append(cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=2 + 10 * s_))
        refs.append(oracle.omp(A, sigs[-1], k, EPS32, nthreads=NT))  # 256 1-GiB sweeps on the host cores
        assert len(refs[-1][0]) == k
    for y, ref in zip(sigs, refs):
        got = d.ctx.omp(y, k, EPS32)
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
    Bd = torch.from_numpy(np.stack(sigs)).cuda()
    idx = torch.full((3, k), -1, dtype=torch.int64, device="cuda")
    val = torch.zeros((3, k), dtype=torch.float64, device="cuda")
    nnz = torch.zeros(3, dtype=torch.int64, device="cuda")
    d.ctx.omp_batch_device(Bd, k, EPS32, idx, val, nnz)
    d.ctx.sync()
    for s_, ref in enumerate(refs):
        assert int(nnz[s_]) == k and np.array_equal(idx[s_].cpu().numpy(), ref[0]) and close(val[s_].cpu().numpy(), ref[1])
    y, xs, ref = sigs[0], planted[0], refs[0]
    full = d.ctx.omp(y, k, EPS32)
    again = d.ctx.omp(y, k, EPS32)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1]) and np.array_equal(full[2], again[2])
    assert len(full[0]) == k and len(np.unique(full[0])) == k and np.all(np.diff(full[0]) > 0)
    # a shorter solve is the prefix of the longer one (OMP is greedy)
    short = d.ctx.omp(y, 12, EPS32)
    assert np.array_equal(short[2], ref[2][:12])
    AS = A[:, full[0]].astype(np.float64)
    r = y - AS @ full[1]
    assert np.abs(AS.T @ r).max() < 1e-10 * np.linalg.norm(y)
    assert np.array_equal(full[0], xs.nzind)  # planted support recovered at this shape
    # sweep linearity: A'(2 r1 - r2) == 2 A'r1 - A'r2 to rounding
    rng = np.random.default_rng(3)
    r1, r2 = rng.standard_normal(M), rng.standard_normal(M)
    c1 = oracle.sweep_abs(A[:, :2048], r1)[0]
    o1, t1, _ = d.ctx.sweep(r1, 1)
    np.testing.assert_allclose(o1[:2048], c1, rtol=1e-11, atol=1e-12)
    assert int(t1[0]) == int(np.argmax(o1))
    d.close()


def test_full_size_config5_gomp_and_sp(cs, oracle):
    """BASELINE configs[4] at its real size (8192 x 131072 f32, 4 GiB): GOMP S=4 k=512 and Subspace Pursuit k=512, every atom
    of the complete solves against the oracle (selection order, support, coefficients to 1e-6, sp's update! count), plus
    size-independent properties: distinct sorted support, least-squares optimality on it (A_S' r = 0), planted recovery,
    idempotent re-run."""
    import torch
    M, N, k, S = 8192, 131072, 512, 4
    g = torch.Generator(device="cuda").manual_seed(4321)
    At = torch.empty((N, M), device="cuda", dtype=torch.float32)
    for lo in range(0, N, 16384):
        a = torch.randn((16384, M), generator=g, device="cuda", dtype=torch.float32)
        At[lo:lo + 16384] = a / a.norm(dim=1, keepdim=True)
    d = cs.Dictionary(At)
    A = np.asfortranarray(At.cpu().numpy().T)
    xs = cs.sparse_vector(N, k, rng=7)
    y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=8)

    ref = oracle.gomp(A, y, S, k, EPS32, nthreads=NT)  # the FULL solve: 128 4-GiB sweeps on the host cores
    full = d.ctx.gomp(y, S, k, EPS32)
    assert len(full[0]) == k and np.all(np.diff(full[0]) > 0)
    assert np.array_equal(full[2], ref[2]) and np.array_equal(full[0], ref[0]) and close(full[1], ref[1])
    got = d.ctx.gomp(y, S, 16, EPS32)  # a shorter solve is the prefix
    assert np.array_equal(got[2], ref[2][:16])
    AS = A[:, full[0]].astype(np.float64)
    r = y - AS @ full[1]
    assert np.abs(AS.T @ r).max() < 1e-10 * np.linalg.norm(y)
    assert np.array_equal(full[0], xs.nzind)  # planted support recovered
    again = d.ctx.gomp(y, S, k, EPS32)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])
    # csmp_gomp_batch (two solves in flight): y and -y have the oracle's support, coefficients of opposite sign
    bi, bv, bn = d.ctx.gomp_batch(np.asfortranarray(np.stack([y, -y], axis=1)), S, k, EPS32)
    assert bn[0] == bn[1] == k and np.array_equal(bi[:k, 0], ref[0]) and np.array_equal(bi[:k, 1], ref[0])
    assert close(bv[:k, 0], ref[1]) and close(-bv[:k, 1], ref[1])

    # Subspace Pursuit, k = 512, complete solves at delta = 1e-2 (stops after the first update!) and at the reference's default
    # 1e-12 (src/twostage.jl:87: iterates until the residual stops decreasing): support, coefficients and the update! count
    for delta in (1e-2, 1e-12):
        rsp = oracle.sp(A, y, k, delta, nthreads=NT)
        gsp = d.ctx.sp(y, k, delta)
        assert gsp[2] == rsp[2] and np.array_equal(gsp[0], rsp[0]) and close(gsp[1], rsp[1]), delta
    big = d.ctx.sp(y, k, 1e-2)
    assert len(big[0]) == k and np.all(np.diff(big[0]) > 0)
    AS = A[:, big[0]].astype(np.float64)
    r = y - AS @ big[1]
    assert np.abs(AS.T @ r).max() < 1e-9 * np.linalg.norm(y)
    assert np.array_equal(big[0], xs.nzind)
    # and a small-k solve on the big dictionary
    xs2 = cs.sparse_vector(N, 24, rng=9)
    y2 = cs.perturb(A[:, xs2.nzind].astype(np.float64) @ xs2.nzval, 5e-3, rng=10)
    rsp = oracle.sp(A, y2, 24, 1e-2, nthreads=NT)
    gsp = d.ctx.sp(y2, 24, 1e-2)
    assert gsp[2] == rsp[2] and np.array_equal(gsp[0], rsp[0]) and close(gsp[1], rsp[1])
    d.close()


_MFMA_SHAPES = [(64, 256, 6, 5), (256, 2048, 12, 40), (130, 700, 10, 130), (512, 4096, 24, 200), (1500, 3000, 16, 9)]
# the provable modes (the defaults, and bf16 operands under the rigorous certificate) on every shape and element type; the opt-in
# statistical certificates -- kept in the library, out of the bench line, breakable on crafted inputs
# (test_batched_certificate_against_adversarial_residuals) -- on two shapes each: they share every kernel but the bound
_MFMA_CASES = [(sh, dt, mode) for mode in ("defaults", "rigorous_bf16") for sh in _MFMA_SHAPES for dt in (np.float32, np.float64)] + \
              [(sh, dt, mode) for mode in ("statistical_f16", "statistical_bf16", "statistical_int8")
               for sh, dt in ((_MFMA_SHAPES[1], np.float32), (_MFMA_SHAPES[3], np.float64))]


@pytest.mark.parametrize("shape,dtype,mode", _MFMA_CASES)
def test_batched_mfma_matches_oracle(cs, oracle, D, shape, dtype, mode):
    """csmp_omp_batch_mfma: MFMA screening (the library's defaults = the rigorous certificate; the opt-in statistical certificates
    with bf16 and int8 operands) + Float64 rescoring must reproduce the oracle's supports exactly and its coefficients to the
    north_star tolerance, signal by signal."""
    n, m, k, nsig = shape
    eps = float(np.finfo(dtype).eps)
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + 3 * m, dtype=dtype)
    d = D(A)
    if mode != "defaults":
        d.ctx.set_option("batch_cert", 1 if mode.startswith("rigorous") else 0)
        d.ctx.set_option("batch_screen", {"int8": 1, "bf16": 0, "f16": 3}[mode.split("_")[1]])
    rng = np.random.default_rng(nsig)
    B = np.asfortranarray(np.stack([cs.perturb(A.astype(np.float64) @ cs.sparse_vector(m, k, rng=rng).to_dense(), 5e-3, rng=rng)
                                    for _ in range(nsig)], axis=1))
    idx, val, nnz = d.ctx.omp_batch_mfma(B, k, eps)
    st = d.ctx.batch_stats()
    assert st["signals"] == nsig and st["illcond"] == 0
    check = range(nsig) if nsig <= 40 else list(range(0, nsig, max(1, nsig // 25)))
    for s in check:
        ref = oracle.omp(A, B[:, s], k, eps)
        assert nnz[s] == len(ref[0]), (s, nnz[s], len(ref[0]))
        assert np.array_equal(idx[:nnz[s], s], ref[0]), (s, idx[:nnz[s], s], ref[0])
        assert close(val[:nnz[s], s], ref[1]), s
    # and it agrees with the exact batch path on every signal
    i2, v2, n2 = d.ctx.omp_batch(B, k, eps)
    assert np.array_equal(nnz, n2) and np.array_equal(idx, i2)
    assert np.allclose(val, v2, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("shape", [(64, 512, 8, np.float32), (50, 301, 5, np.float64), (256, 2048, 24, np.float32)])
def test_streamed_dictionary_and_dictionary_files(cs, oracle, shape, tmp_path):
    """SURVEY §8(f-4), second half: a dictionary that stays in HOST memory (CSMP_HOST_STREAMED: every kernel reads A over the host
    link -- the mode for a dictionary larger than HBM) and dictionary files read into HBM or into mapped host memory.  All of them
    must return what the resident dictionary returns: the oracle's supports, coefficients to the north_star tolerance -- for omp,
    gomp, sp and the batched path.  (64 / 256 rows: the array is registered where it lies; 50 rows: padded page-locked copy.)"""
    n, m, k, dtype = shape
    eps = float(np.finfo(dtype).eps)
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=3 * n + m, dtype=dtype)
    path = str(tmp_path / "dict.csmp")
    cs.write_dictionary_file(path, A)
    assert cs.dictionary_file_info(path) == (n, m, dtype)
    variants = {"resident": cs.Dictionary(A), "streamed": cs.Dictionary(A, streamed=True),
                "file_resident": cs.Dictionary(path), "file_streamed": cs.Dictionary(path, streamed=True)}
    ref = oracle.omp(A, b, k, eps)
    refg = oracle.gomp(A, b, 2, k, eps)
    refs = oracle.sp(A, b, min(k, n // 2), 1e-9)
    rng = np.random.default_rng(n)
    B = np.asfortranarray(np.stack([cs.perturb(A.astype(np.float64) @ cs.sparse_vector(m, k, rng=rng).to_dense(), 5e-3, rng=rng)
                                    for _ in range(4)], axis=1))
    base = None
    for name, d in variants.items():
        assert d.shape == (n, m) and d.dtype == np.dtype(dtype), name
        g = d.ctx.omp(b, k, eps)
        assert np.array_equal(g[0], ref[0]) and close(g[1], ref[1]), name
        gg = d.ctx.gomp(b, 2, k, eps)
        assert np.array_equal(gg[0], refg[0]) and close(gg[1], refg[1]), name
        gs = d.ctx.sp(b, min(k, n // 2), 1e-9)
        assert np.array_equal(gs[0], refs[0]) and close(gs[1], refs[1]), name
        idx, val, nnz = d.ctx.omp_batch_mfma(B, k, eps)
        sb = d.ctx.sp_batch(B, min(k, n // 2), 1e-9)  # (several solves in flight: clones of the context share the mapped dictionary)
        if base is None:
            base = (idx, val, nnz, sb)
        else:  # bit for bit the resident dictionary's results
            assert np.array_equal(idx, base[0]) and np.array_equal(nnz, base[2]) and np.array_equal(val, base[1]), name
            assert all(np.array_equal(u, v) for u, v in zip(sb, base[3])), name
    for d in variants.values():
        d.close()
    with pytest.raises(cs.CsmpError):
        cs.Dictionary(str(tmp_path / "missing.csmp"))


def test_batched_mfma_beyond_8192_rows_runs_the_exact_batch(cs, oracle, D):
    """include/csmp.h: a dictionary of more than 8192 rows (the per-signal kernels' register/LDS budget) is not refused: the call
    returns csmp_omp_batch's results (the contract) and reports that no screening kernel ran."""
    n, m, k, nsig = 8200, 1024, 6, 5
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=5, dtype=np.float32)
    d = D(A)
    rng = np.random.default_rng(6)
    B = np.asfortranarray(np.stack([cs.perturb(A.astype(np.float64) @ cs.sparse_vector(m, k, rng=rng).to_dense(), 5e-3, rng=rng)
                                    for _ in range(nsig)], axis=1))
    eps = float(np.finfo(np.float32).eps)
    idx, val, nnz = d.ctx.omp_batch_mfma(B, k, eps)
    st = d.ctx.batch_stats()
    assert st["signals"] == nsig and st["resolved_exactly"] == 0
    assert d.ctx.batch_screen_kernel().startswith("none")
    for s in range(nsig):
        ref = oracle.omp(A, B[:, s], k, eps)
        assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]) and close(val[:nnz[s], s], ref[1])
    d.close()


def test_batched_mfma_at_the_reference_default_capacity(cs, oracle, D):
    """omp(A, b) defaults to k = size(A, 1) (src/matchingpursuit.jl:89): the batched path must take that capacity -- through its own
    kernels where the per-signal vectors fit the LDS (k = M = 2048), through csmp_omp_batch's exact sweeps where they do not
    (k = M = 5632) -- and stop by eps after the planted atoms either way."""
    for n, m, mode in ((2048, 2304, "screen"), (5632, 5760, "none")):
        A, x, b = cs.sparse_data(n=n, m=m, k=5, rng=n, dtype=np.float32)
        d = D(A)
        rng = np.random.default_rng(n + 1)
        B = np.asfortranarray(np.stack([A.astype(np.float64) @ cs.sparse_vector(m, 5, rng=rng).to_dense() for _ in range(3)], axis=1))
        idx, val, nnz = d.ctx.omp_batch_mfma(B, n, 1e-5)
        assert d.ctx.batch_screen_kernel().startswith("none") == (mode == "none")
        for s in range(3):
            ref = oracle.omp(A, B[:, s], n, 1e-5)
            assert nnz[s] == len(ref[0]) == 5 and np.array_equal(idx[:5, s], ref[0]) and close(val[:5, s], ref[1])
        d.close()


def test_batched_mfma_solves_in_chunks_when_hbm_is_short(cs, oracle, D):
    """The per-signal state of the batched path grows with k^2 (two k x k Float64 factors per signal): a batch that does not fit
    the free HBM is solved in chunks of whole 256-signal tiles, with csmp_omp_batch's results.  The GPU's memory is filled up to
    the planner's HBM budget is lowered through the test hook (csmp_tune: batch_budget_mib) so that a small batch meets the situation a
    288 GB device meets at k in the thousands -- without exhausting the physical memory of a shared device."""
    n, m, k, nsig = 512, 2048, 512, 600
    A, x, b = cs.sparse_data(n=n, m=m, k=6, rng=9, dtype=np.float32)
    d = D(A)
    rng = np.random.default_rng(10)
    B = np.asfortranarray(np.stack([cs.perturb(A.astype(np.float64) @ cs.sparse_vector(m, 6, rng=rng).to_dense(), 5e-3, rng=rng)
                                    for _ in range(nsig)], axis=1))
    eps = 5e-2  # (stops after the planted atoms: the CAPACITY k = 512 is what sizes the state)
    i0, v0, n0 = d.ctx.omp_batch(B, k, eps)
    d.ctx.omp_batch_mfma(B[:, :8], 4, eps)  # (the operand image exists before the memory is measured)
    per = 2 * k * k * 8
    d.ctx.tune("batch_budget_mib", (300 * per) >> 20)  # room for one 256-signal tile, not for two
    try:
        idx, val, nnz = d.ctx.omp_batch_mfma(B, k, eps)
        st = d.ctx.batch_stats()
    finally:
        d.ctx.tune("batch_budget_mib", 0)
    assert st["signals"] == nsig and d.ctx.batch_screen_kernel().startswith("csmp::k_b_screen")
    assert np.array_equal(nnz, n0) and np.array_equal(idx, i0) and np.allclose(val, v0, rtol=1e-9, atol=1e-12)
    assert d.ctx.batch_layout()["screen_signals"] == 256  # signal columns of the last screening launch: one tile, i.e. the batch went in pieces
    for s in (0, 255, 256, 511, 512, nsig - 1):
        ref = oracle.omp(A, B[:, s], k, eps)
        assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]) and close(val[:nnz[s], s], ref[1])
    d.close()


def test_c_program_through_the_abi(cs, tmp_path):
    """tests/c_abi_example.c (plain C99 on include/csmp.h): omp, gomp, omp_batch and a dictionary file round trip, with the
    supports the numpy oracle gives for its dictionary hard-coded inside.  Exit code 0 = every check held."""
    import subprocess
    from test_abi import build_c_example
    exe = build_c_example(cs, str(tmp_path / "c_abi_example"))
    r = subprocess.run([exe, str(tmp_path / "c_example.csmp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_batched_mfma_eps_stop_and_padding(cs, oracle, D):
    # noiseless 3-sparse signals, k = 8: every signal stops after 3 atoms (eps-stop inside k_b_step)
    A, x, b = cs.sparse_data(n=96, m=400, k=3, rng=1, dtype=np.float32)
    d = D(A)
    rng = np.random.default_rng(2)
    B = np.asfortranarray(np.stack([A.astype(np.float64) @ cs.sparse_vector(400, 3, rng=rng).to_dense() for _ in range(7)], axis=1))
    idx, val, nnz = d.ctx.omp_batch_mfma(B, 8, 1e-6)
    for s in range(7):
        ref = oracle.omp(A, B[:, s], 8, 1e-6)
        assert nnz[s] == len(ref[0]) == 3 and np.array_equal(idx[:3, s], ref[0]) and close(val[:3, s], ref[1])
        assert np.all(idx[3:, s] == -1)
    with pytest.raises(cs.CsmpError):
        d.ctx.omp_batch_mfma(B, 8, -1.0)
    # a location code that is not CSMP_HOST / CSMP_DEVICE is refused, not dereferenced (CSMP_HOST_STREAMED belongs to dictionaries)
    import ctypes as C
    Bf = np.asfortranarray(B)
    idx = np.zeros((8, 7), np.int64, order="F")
    val = np.zeros((8, 7), np.float64, order="F")
    nn = np.zeros(7, np.int64)
    for name in ("csmp_omp_batch", "csmp_omp_batch_mfma"):
        with pytest.raises(cs.CsmpError):
            d.ctx.call(name, Bf.ctypes.data_as(C.c_void_p), 1, C.c_int64(96), C.c_int64(7), 2, C.c_int64(8), C.c_double(1e-6),
                       idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), nn.ctypes.data_as(C.c_void_p), 0)


def test_oblivious_and_acquisitions(cs, oracle, D):
    # src/oblivious.jl:3-8: top-k of |A'b| then least squares on those columns
    A, x, b = cs.sparse_data(n=64, m=300, k=5, rng=31, dtype=np.float32)
    y = cs.perturb(b, 5e-3, rng=32)
    d = D(A)
    xo = cs.oblivious(d, y, 5)
    top = oracle.topk_desc(oracle.sweep_abs(A, y)[0], 5)
    assert np.array_equal(xo.nzind, np.sort(top))
    ref = np.linalg.lstsq(A[:, np.sort(top)].astype(np.float64), y, rcond=None)[0]
    assert close(xo.nzval, ref)
    xa = cs.oblivious_acquisition(d, y, cs.spzeros(300), 5)  # src/matchingpursuit.jl:207-216 on an empty x
    assert np.array_equal(xa.nzind, xo.nzind) and close(xa.nzval, ref)
    xr = cs.random_acquisition(d, y, cs.spzeros(300), 6, rng=1)  # :195-204
    assert xr.nnz == 6 and close(xr.nzval, np.linalg.lstsq(A[:, xr.nzind].astype(np.float64), y, rcond=None)[0])
    xs = cs.omp_batch_mfma(d, np.stack([y, y], axis=1), 5)
    r = oracle.omp(A, y, 5, EPS32)
    assert np.array_equal(xs[0].nzind, r[0]) and close(xs[1].nzval, r[1])


@pytest.mark.parametrize("cfg", [(2048, 3000, 12, 7, np.float32), (4096, 2500, 10, 5, np.float32), (1024, 1500, 9, 4, np.float64),
                                 (2048, 1000, 8, 8, np.float64), (512, 900, 6, 6, np.float32)])
def test_pipelined_batch_matches_oracle(cs, oracle, D, cfg):
    """csmp_omp_batch takes signals three at a time through k_tick (sweep of one signal fused with the
    append stages of two others).  Shapes chosen so that the software-pipelined sweep body (U = 8 / 16)
    and the plain one are both exercised; group sizes 3, 2 and 1 all occur."""
    n, m, k, nsig, dtype = cfg
    eps = float(np.finfo(dtype).eps)
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m, dtype=dtype)
    d = D(A)
    rng = np.random.default_rng(nsig)
    B = np.asfortranarray(np.stack([cs.perturb(A[:, (xs := cs.sparse_vector(m, k, rng=rng)).nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=rng)
                                    for _ in range(nsig)], axis=1))
    idx, val, nnz = d.ctx.omp_batch(B, k, eps)
    for s in range(nsig):
        ref = oracle.omp(A, B[:, s], k, eps)
        assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]), s
        assert close(val[:nnz[s], s], ref[1]), s
        solo = d.ctx.omp(B[:, s], k, eps)  # the one-at-a-time chain gives bit-identical numbers
        assert np.array_equal(solo[0], idx[:nnz[s], s]) and np.array_equal(solo[1], val[:nnz[s], s])


def test_edge_cases_tiny_and_degenerate(cs, oracle, D):
    """Sizes at the edges of every kernel's indexing: one row, one atom, k = 0, k > N, k > M."""
    rng = np.random.default_rng(0)
    # k = 0: nothing selected
    A, x, b = cs.sparse_data(n=16, m=24, k=2, rng=1)
    d = D(A)
    i, v, o = d.ctx.omp(b, 0, 0.0)
    assert len(i) == 0
    assert len(d.ctx.mp(b, 0)[0]) == 0
    # k larger than the number of atoms: every atom gets selected once, then stagnation (:66)
    A3 = np.asfortranarray(rng.standard_normal((12, 3)))
    A3 /= np.linalg.norm(A3, axis=0)
    b3 = rng.standard_normal(12)
    d3 = D(A3)
    ref = oracle.omp(A3, b3, 7, 0.0)
    got = d3.ctx.omp(b3, 7, 0.0)
    assert np.array_equal(got[0], ref[0]) and len(got[0]) == 3 and close(got[1], ref[1])
    # one atom, one row
    A1 = np.asfortranarray(np.array([[2.0]]))
    d1 = D(A1)
    got = d1.ctx.omp(np.array([3.0]), 1, 0.0)
    assert got[0].tolist() == [0] and abs(got[1][0] - 1.5) < 1e-15
    # M = 2 rows, k > M: support fills the row space then stops (:63)
    A2 = np.asfortranarray(rng.standard_normal((2, 9)).astype(np.float32))
    b2 = rng.standard_normal(2)
    d2 = D(A2)
    ref = oracle.omp(A2, b2, 5, 0.0)
    got = d2.ctx.omp(b2, 5, 0.0)
    assert np.array_equal(got[0], ref[0]) and len(got[0]) == 2
    # gomp with l > k and l > N
    ref = oracle.gomp(A3, b3, 5, 2, 0.0)
    got = d3.ctx.gomp(b3, 5, 2, 0.0)
    assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
    # batch of one signal, batch with k = 1
    idx, val, nnz = d.ctx.omp_batch(np.asfortranarray(b[:, None]), 1, 0.0)
    assert nnz[0] == 1 and idx[0, 0] == oracle.omp(A, b, 1, 0.0)[0][0]
    idx, val, nnz = d.ctx.omp_batch_mfma(np.asfortranarray(np.stack([b, 2 * b], axis=1)), 2, 0.0)
    r2 = oracle.omp(A, b, 2, 0.0)
    assert np.array_equal(idx[:, 0], r2[0]) and np.array_equal(idx[:, 1], r2[0]) and close(val[:, 1], 2 * r2[1])


def test_block_append_falls_back_on_coherent_panels(cs, oracle, D):
    """Multi-column append (GOMP panels, SP / lstsq factorisations): on a highly coherent dictionary a
    panel fails its DGKS test, nothing is committed and the host repeats the solve column-wise with
    re-orthogonalisation.  Results must still match the oracle (tolerance scaled by conditioning)."""
    rng = np.random.default_rng(8)
    n, m = 96, 260
    U, V = rng.standard_normal((n, n)), rng.standard_normal((n, m))
    A = (U * (1.0 / np.arange(1, n + 1) ** 2)) @ V
    A /= np.linalg.norm(A, axis=0)
    A = np.asfortranarray(A)
    d = D(A)
    xs = cs.sparse_vector(m, 6, rng=rng)
    y = cs.perturb(A @ xs.to_dense(), 1e-3, rng=rng)
    ref = oracle.gomp(A, y, 3, 6, EPS64)
    got = d.ctx.gomp(y, 3, 6, EPS64)
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0])
    cond = np.linalg.cond(A[:, ref[0]])
    assert np.allclose(got[1], ref[1], rtol=1e-6, atol=1e-11 * cond * np.abs(ref[1]).max()), cond
    cols = np.array([5, 6, 7, 8, 9, 100, 101, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52,
                     53, 54, 55, 56, 57, 58, 59, 60, 61, 62])  # 40 columns: two panels
    got = d.ctx.lstsq(cols, y)
    want = np.linalg.lstsq(A[:, cols], y, rcond=None)[0]
    cond = np.linalg.cond(A[:, cols])
    r1, r2 = y - A[:, cols] @ got, y - A[:, cols] @ want
    assert abs(np.linalg.norm(r1) - np.linalg.norm(r2)) <= 1e-9 * np.linalg.norm(y) * max(1.0, cond * 1e-6), (cond,)
    # well-conditioned panels on the same context still take the fast path and agree tightly
    A2, x2, b2 = cs.sparse_data(n=96, m=260, k=5, rng=3)
    d2 = D(A2)
    cols2 = np.arange(0, 70, 2)
    np.testing.assert_allclose(d2.ctx.lstsq(cols2, b2), np.linalg.lstsq(A2[:, cols2], b2, rcond=None)[0], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("cfg", [(32, 64, 3, np.float64), (128, 512, 12, np.float32), (100, 333, 9, np.float64), (256, 2048, 40, np.float32)])
def test_ompr_matches_oracle(cs, oracle, D, cfg):
    """OMP with replacement (src/twostage.jl:110-202): same supports, coefficients and number of
    update! calls as the oracle, noiseless and noisy; property of test/twostage.jl on the way."""
    n, m, k, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m + 1, dtype=dtype)
    d = D(A)
    for y, delta in ((b, 1e-6), (cs.perturb(b, 5e-3, rng=2), 1e-2), (cs.perturb(b, 5e-2, rng=3), 1e-6)):
        ref = oracle.ompr(A, y, k, delta)
        got = d.ctx.ompr(y, k, delta)
        assert got[2] == ref[2], ("update! calls", got[2], ref[2])
        assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
    xo = cs.ompr(d, b, k, 1e-6)
    assert np.array_equal(xo.nzind, oracle.ompr(A, b, k, 1e-6)[0])


def test_near_tie_below_f32_resolution_is_resolved_in_f64(cs, oracle, D):
    """Two atoms whose correlations with r differ by ~1e-9 relative -- far below what an f32 (or
    bf16) accumulation can resolve -- with the LARGER one at the HIGHER index, so that a low-precision
    tie would be broken the wrong way (lowest index).  The Float64 sweep, and the batched path's
    Float64 rescoring of the bf16-screened candidates, must both pick the oracle's atom."""
    rng = np.random.default_rng(123)
    M, N = 512, 3000
    A = rng.standard_normal((M, N)).astype(np.float32)
    A /= np.linalg.norm(A, axis=0).astype(np.float32)
    lo, hi = 700, 2100
    A[:, hi] = A[:, lo]
    r = rng.standard_normal(M) + 40.0 * A[:, lo].astype(np.float64)  # makes both copies the clear arg-max pair
    m = int(np.argmax(np.abs(r) * np.abs(A[:, lo])))  # a row where a one-ulp nudge is felt
    c_lo = float(A[:, lo].astype(np.float64) @ r)
    A[m, hi] = np.nextafter(A[m, hi], np.float32(np.inf if c_lo * r[m] > 0 else -np.inf))  # grows |<a_hi, r>|
    A = np.asfortranarray(A)
    c = A.astype(np.float64).T @ r
    assert abs(c[hi]) > abs(c[lo]) and (abs(c[hi]) - abs(c[lo])) / abs(c[hi]) < 1e-7
    d = D(A)
    out, ti, tv = d.ctx.sweep(r, 2)
    assert ti.tolist() == [hi, lo]
    ref = oracle.omp(A, r, 3, 0.0)
    got = d.ctx.omp(r, 3, 0.0)
    assert got[2][0] == hi == ref[2][0] and np.array_equal(got[2], ref[2]) and close(got[1], ref[1])
    idx, val, nnz = d.ctx.omp_batch_mfma(np.asfortranarray(np.stack([r, 0.5 * r], axis=1)), 3, 0.0)
    assert np.array_equal(np.sort(idx[:, 0]), ref[0]) and np.array_equal(np.sort(idx[:, 1]), ref[0])
    assert close(val[:, 0], ref[1])


# ------------------------------------------------------------------------------------------------
# forward regression / orthogonal least squares (fr = ols = oomp = ormp; src/forward.jl)
@pytest.mark.parametrize("shape", [(32, 48, 3), (64, 256, 8), (37, 101, 5), (256, 1024, 32), (130, 700, 20), (512, 4096, 40),
                                   (1024, 2000, 24), (2048, 1500, 16), (4096, 1200, 12)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fr_matches_oracle(cs, oracle, D, shape, dtype):
    n, m, k = shape
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n * 17 + m, dtype=dtype)
    d = D(A)
    for seed in range(2):
        xs = cs.sparse_vector(m, k, rng=seed)
        y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=seed + 100)
        ref = oracle.fr(A, y, k)
        got = d.ctx.fr(y, k)
        assert np.array_equal(got[2], ref[2]), "selection order"
        assert np.array_equal(got[0], ref[0])
        assert close(got[1], ref[1])
    # the public driver: fr(A, b, sparsity = k) and the aliases (test/forward.jl:15-22)
    xg = cs.fr(d, y, sparsity=k)
    assert np.array_equal(xg.nzind, ref[0]) and close(xg.nzval, ref[1])
    assert cs.ols is cs.fr and cs.oomp is cs.fr and cs.ormp is cs.fr


def test_fr_reference_known_answer(cs, D):
    """test/forward.jl:14-22 on seeded data: planted 3-sparse recovery, noiseless and perturbed."""
    ok = 0
    for seed in range(10):
        A, x, b = cs.sparse_data(n=32, m=48, k=3, rng=seed)
        d = D(A)
        xfr = cs.fr(d, b, sparsity=3)
        y = cs.perturb(b, 1e-2, rng=seed)
        yfr = cs.fr(d, y, sparsity=3)
        ok += (np.array_equal(xfr.nzind, x.nzind) and np.allclose(xfr.nzval, x.nzval)
               and np.array_equal(yfr.nzind, x.nzind) and np.allclose(yfr.nzval, x.nzval, atol=2e-2))
    assert ok >= 9  # "may rarely fail" on random data (test/matchingpursuit.jl:7)


def test_fr_stopping_rules(cs, oracle, D):
    A, x, b = cs.sparse_data(n=256, m=1024, k=24, rng=5, dtype=np.float32)
    y = cs.perturb(b, 5e-3, rng=6)
    d = D(A)
    # residual tolerance: norm(r) > max_eps || return false (src/forward.jl:60-61)
    for max_eps in (0.5, 0.05, 6e-3):
        ref = oracle.fr(A, y, 100, max_eps=max_eps)
        got = d.ctx.fr(y, 100, max_eps, 0.0)
        assert np.array_equal(got[2], ref[2]) and close(got[1], ref[1]) and 0 < len(got[0]) < 100
    # marginal decrease: the step fails unless min_delta^2 < max δ² (:64)
    for min_delta in (0.9, 0.3, 0.01):
        ref = oracle.fr(A, y, 100, min_delta=min_delta)
        got = d.ctx.fr(y, 100, 0.0, min_delta)
        assert np.array_equal(got[2], ref[2]) and close(got[1], ref[1]) and len(got[0]) < 100
    assert len(d.ctx.fr(y, 100, 0.0, 1e3)[0]) == 0 and len(oracle.fr(A, y, 100, min_delta=1e3)[0]) == 0
    assert len(d.ctx.fr(y, 100, 1e3, 0.0)[0]) == 0
    assert len(d.ctx.fr(y, 0)[0]) == 0
    # keyword form (:34-37) and positional form (:44-45, k defaults to size(A,1))
    xk = cs.fr(d, y, max_residual=0.05, min_decrease=0.01, sparsity=50)
    ref = oracle.fr(A, y, 50, max_eps=0.05, min_delta=0.01)
    assert np.array_equal(xk.nzind, ref[0]) and close(xk.nzval, ref[1])
    xp = cs.fr(d, y, 0.05, 0.01)
    assert np.array_equal(xp.nzind, ref[0])
    # nnz(x) < size(A,1) guard (:58): a square-ish system fills up and stops at M atoms
    A2, _, b2 = cs.sparse_data(n=12, m=40, k=3, rng=9)
    y2 = cs.perturb(b2, 1e-1, rng=1)
    got = D(A2).ctx.fr(y2, 30)
    ref = oracle.fr(A2, y2, 30)
    assert len(ref[0]) <= 12 and np.array_equal(got[2][:8], ref[2][:8])
    with pytest.raises(ValueError):
        cs.fr(d, y[:-1], sparsity=3)


def test_fr_scores_and_functor(cs, oracle, D):
    """update!(P::FR, x) step by step (src/forward.jl:88-95) and P.δ² (:75-82) against the formula
    evaluated from scratch in numpy: <a_j,r>^2 / (|a_j|^2 - |Q'a_j|^2), zero on the support."""
    A, x, b = cs.sparse_data(n=96, m=400, k=6, rng=2)
    y = cs.perturb(b, 1e-2, rng=3)
    d = D(A)
    P = cs.FR(d, y)
    xg = cs.spzeros(400)
    ref_order = oracle.fr(A, y, 6)[2]
    supp = []
    for t in range(6):
        if supp:
            S = np.array(sorted(supp))
            coef = np.linalg.lstsq(A[:, S], y, rcond=None)[0]
            r = y - A[:, S] @ coef
            Q = np.linalg.qr(A[:, S])[0]
            resc = np.sum(A * A, axis=0) - np.sum((Q.T @ A) ** 2, axis=0)
        else:
            r, resc = y.copy(), np.sum(A * A, axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = (A.T @ r) ** 2 / resc
        want[supp] = 0.0
        xg = P(xg)
        got = P.delta2
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12 * want.max())
        assert int(np.argmax(want)) == ref_order[t] == P.order[t]
        supp.append(int(ref_order[t]))
    assert np.array_equal(xg.nzind, np.sort(ref_order))
    assert close(xg.nzval, np.linalg.lstsq(A[:, xg.nzind], y, rcond=None)[0])
    assert cs.OLS is cs.FR


def test_fr_differs_from_omp_on_coherent_dictionary(cs, oracle, D):
    """OLS and OMP part ways when atoms are correlated with the selected ones: the parity check must
    follow the OLS rule, not the OMP one.  Dictionary with a strong common component."""
    rng = np.random.default_rng(11)
    M, N, k = 48, 600, 16
    A = rng.standard_normal((M, N)) + 1.5 * rng.standard_normal((M, 1))
    A /= np.linalg.norm(A, axis=0)
    b = A[:, rng.choice(N, k, replace=False)] @ rng.standard_normal(k) + 1e-3 * rng.standard_normal(M)
    d = D(A)
    ref = oracle.fr(A, b, k)
    got = d.ctx.fr(b, k)
    assert np.array_equal(got[2], ref[2]) and close(got[1], ref[1], tight=False)
    assert not np.array_equal(oracle.omp(A, b, k, 0.0)[2], ref[2])


def test_fr_duplicate_columns_tie_goes_to_lowest_index(cs, oracle, D):
    A, x, b = cs.sparse_data(n=64, m=200, k=4, rng=3, dtype=np.float32)
    A = np.asfortranarray(A)
    first = int(oracle.fr(A, b, 1)[2][0])
    dup = (first + 57) % 200
    A[:, dup] = A[:, first]
    lo = min(first, dup)
    got = D(A).ctx.fr(b, 1)
    assert got[2][0] == lo == oracle.fr(A, b, 1)[2][0]


def test_full_size_config2_forward_regression(cs, oracle):
    """C2 shape (4096 x 65536 f32): 48 OLS steps against the oracle (support, order, coefficients) and
    the defining property of every OLS solution: the residual is orthogonal to the selected atoms."""
    M, N, k = 4096, 65536, 48
    A, x, b = cs.sparse_data(n=M, m=N, k=k, rng=77, dtype=np.float32)
    y = cs.perturb(b, 5e-3, rng=78)
    d = cs.Dictionary(A)
    try:
        got = d.ctx.fr(y, k)
        ref = oracle.fr(A, y, k)
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
        r = y - A[:, got[0]].astype(np.float64) @ got[1]
        assert np.max(np.abs(A[:, got[0]].astype(np.float64).T @ r)) < 1e-12
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------
# column removal from the on-device QR (remove_column! / dropindex!, src/util.jl:137-161)
@pytest.mark.parametrize("cfg", [(100, 300, 12, np.float64), (256, 1000, 40, np.float32), (77, 200, 9, np.float32),
                                 (1024, 3000, 150, np.float32)])
def test_qr_column_removal(cs, D, cfg):
    """Build a support with OMP steps, remove atoms at the first / a middle / the last insertion
    position, and after every removal compare coefficients and residual with a dense least-squares
    solve on what is left; then keep stepping (appends on top of a down-dated factorisation)."""
    n, m, k, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + k, dtype=dtype)
    y = cs.perturb(b, 5e-2, rng=1)
    d = D(A)
    A64 = A.astype(np.float64)
    d.ctx.solver_begin(cs._lib.ALGO_OMP, y, k + 2)
    for _ in range(k):
        d.ctx.solver_step(1)
    idx, val, res, order, stop = d.ctx.solver_state(k + 2)
    assert len(idx) == k

    def check(expect_support):
        idx, val, res, order, stop = d.ctx.solver_state(k + 2)
        S = np.array(sorted(expect_support))
        assert np.array_equal(idx, S)
        coef = np.linalg.lstsq(A64[:, S], y, rcond=None)[0]
        assert close(val, coef, tight=False) and np.allclose(val, coef, rtol=1e-8, atol=1e-10)
        assert np.isclose(res, np.linalg.norm(y - A64[:, S] @ coef), rtol=1e-8, atol=1e-12)
        return order

    supp = list(order)
    for pos in (0, len(supp) // 2, -1, 1):
        atom = supp[pos]
        d.ctx.solver_remove(atom)
        supp.remove(atom)
        order = check(supp)
        assert list(order) == supp  # insertion order is preserved among the survivors
    d.ctx.solver_remove(10 ** 6)  # not in the support: no-op
    check(supp)
    for _ in range(3):  # appends after removals
        d.ctx.solver_step(1)
        idx, val, res, order, stop = d.ctx.solver_state(k + 2)
        supp = list(order)
        check(supp)
    # remove everything, one by one
    for atom in list(supp):
        d.ctx.solver_remove(atom)
        supp.remove(atom)
        if supp:
            check(supp)
    idx, val, res, order, stop = d.ctx.solver_state(k + 2)
    assert len(idx) == 0 and np.isclose(res, np.linalg.norm(y), rtol=1e-10)


def test_qr_column_removal_beyond_1023_columns(cs, D):
    """dropindex! has no column cap in the reference (src/util.jl:137-161); rounds 1-4 stopped the step-level csmp_solver_remove at
    1023 columns (one thread per column in k_qrdel_r).  A 2048-column support (built by oblivious_acquisition!, then update!s):
    removals at the first / a middle / the last / the second insertion position, each checked against a dense least-squares solve,
    insertion order preserved, appends on top of the down-dated factorisation, an absent atom a no-op."""
    M, N, k = 4096, 6000, 2048
    g = np.random.default_rng(2048)
    A = g.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    A = np.asfortranarray(A.astype(np.float32))
    A64 = A.astype(np.float64)
    y = A64[:, g.choice(N, 64, replace=False)] @ g.standard_normal(64) + 0.05 * g.standard_normal(M)
    d = D(A)
    d.ctx.solver_begin(cs._lib.ALGO_OMP, y, k + 8)
    d.ctx.solver_acquire(k - 2)
    for _ in range(2):
        d.ctx.solver_step(1)
    idx, val, res, order, stop = d.ctx.solver_state(k + 8)
    assert len(idx) == k

    def check(expect_support):
        idx, val, res, order, stop = d.ctx.solver_state(k + 8)
        S = np.array(sorted(expect_support))
        assert np.array_equal(idx, S)
        coef = np.linalg.lstsq(A64[:, S], y, rcond=None)[0]
        assert np.allclose(val, coef, rtol=1e-7, atol=1e-9 * np.abs(coef).max())
        assert np.isclose(res, np.linalg.norm(y - A64[:, S] @ coef), rtol=1e-8, atol=1e-12)
        return order

    supp = list(order)
    for pos in (0, len(supp) // 2, -1, 1):
        atom = supp[pos]
        d.ctx.solver_remove(atom)
        supp.remove(atom)
        order = check(supp)
        assert list(order) == supp
    d.ctx.solver_remove(10 ** 6)
    check(supp)
    for _ in range(2):
        d.ctx.solver_step(1)
    idx, val, res, order, stop = d.ctx.solver_state(k + 8)
    assert len(idx) == k - 2
    check(list(order))


def test_qr_column_removal_at_the_reference_default_capacity(cs, D):
    """GOMP(A, b, l) defaults its capacity to size(A, 1) (src/matchingpursuit.jl:108): at M = 4608 that is beyond the 4095 columns the
    rotation kernels scan, and dropindex! must still work (src/util.jl:137-161 has no cap): the factorisation is rebuilt without
    the atom.  Removals, then appends on top, each state against a dense least-squares solve."""
    M, N = 4608, 5000
    g = np.random.default_rng(4608)
    A = g.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    A = np.asfortranarray(A.astype(np.float32))
    A64 = A.astype(np.float64)
    y = A64[:, g.choice(N, 20, replace=False)] @ g.standard_normal(20) + 0.05 * g.standard_normal(M)
    d = D(A)
    d.ctx.solver_begin(cs._lib.ALGO_GOMP, y, M)  # the reference's default capacity
    for _ in range(6):
        d.ctx.solver_step(4)
    idx, val, res, order, stop = d.ctx.solver_state(M)
    supp = list(order)
    assert len(supp) == 24
    for pos in (0, 11, -1):
        atom = supp[pos]
        d.ctx.solver_remove(atom)
        supp.remove(atom)
        idx, val, res, order, stop = d.ctx.solver_state(M)
        assert list(order) == supp and np.array_equal(idx, np.array(sorted(supp)))
        coef = np.linalg.lstsq(A64[:, idx], y, rcond=None)[0]
        assert np.allclose(val, coef, rtol=1e-8, atol=1e-10) and np.isclose(res, np.linalg.norm(y - A64[:, idx] @ coef), rtol=1e-8)
    d.ctx.solver_remove(10 ** 6)
    d.ctx.solver_step(4)
    idx, val, res, order, stop = d.ctx.solver_state(M)
    assert len(idx) == 25 and list(order)[:21] == supp
    coef = np.linalg.lstsq(A64[:, idx], y, rcond=None)[0]
    assert np.allclose(val, coef, rtol=1e-8, atol=1e-10)


# ------------------------------------------------------------------------------------------------
# stepwise regression with replacement (srr, src/twostage.jl:3-33): forward steps + backward steps
@pytest.mark.parametrize("cfg", [(32, 64, 3, 1, np.float64), (32, 64, 3, 3, np.float64), (128, 512, 12, 1, np.float32),
                                 (128, 512, 8, 4, np.float32), (100, 333, 9, 2, np.float64), (256, 2048, 24, 1, np.float32),
                                 (512, 4096, 40, 1, np.float32), (1024, 3000, 30, 5, np.float32)])
@pytest.mark.parametrize("init", [1, 2])
def test_srr_matches_oracle(cs, oracle, D, cfg, init):
    n, m, k, l, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m + k, dtype=dtype)
    d = D(A)
    for seed, noise in ((0, 0.0), (1, 5e-3), (2, 2e-1)):  # the noisy cases make the replacement loop work
        xs = cs.sparse_vector(m, k + 2, rng=seed)  # two atoms more than srr may keep
        y = A[:, xs.nzind].astype(np.float64) @ xs.nzval
        if noise:
            y = cs.perturb(y, noise, rng=seed + 50)
        ref = oracle.srr(A, y, k, 1e-12, -1, init, l)
        got = d.ctx.srr(y, k, 1e-12, -1, init, l)
        assert np.array_equal(got[0], ref[0]), (seed, got, ref)
        assert close(got[1], ref[1], tight=False)
        assert got[2] == ref[2], "iterations"
    xg = cs.srr(d, y, k, initialization=init, l=l)
    assert np.array_equal(xg.nzind, ref[0])


@pytest.mark.parametrize("cfg", [(32, 64, 3, 1, np.float64), (128, 512, 12, 2, np.float32), (256, 2048, 24, 1, np.float32)])
def test_srr_random_initialization(cs, oracle, D, cfg):
    """srr(initialization = 3), src/twostage.jl:14-16: random_acquisition! (src/matchingpursuit.jl:195-204) with the draw made by
    the caller -- csmp_srr_from -- against the oracle on the same draw; the Python mirror draws from a seeded Generator."""
    n, m, k, l, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m + k, dtype=dtype)
    y = cs.perturb(b, 5e-3, rng=3)
    d = D(A)
    for seed in range(4):
        init = np.random.default_rng(seed).choice(m, size=k, replace=False)
        ref = oracle.srr(A, y, k, 1e-12, -1, 3, l, init=init)
        got = d.ctx.srr(y, k, 1e-12, -1, 3, l, init)
        assert np.array_equal(got[0], ref[0]), (seed, got, ref)
        assert close(got[1], ref[1], tight=False)
        assert got[2] == ref[2], "iterations"
        xs = cs.srr(d, y, k, initialization=3, l=l, rng=seed)  # the mirror's own draw: the same Generator, the same atoms
        assert np.array_equal(xs.nzind, ref[0])
    with pytest.raises(cs.CsmpError):
        d.ctx.srr(y, k, 1e-12, -1, 3, l, np.zeros(k, np.int64))  # duplicates (k > 1) / k = 1: a valid single atom
    with pytest.raises(cs.CsmpError):
        d.ctx.srr(y, k, 1e-12, -1, 3, l, np.full(k, m, np.int64) + np.arange(k))  # out of range


def test_srr_reference_known_answer(cs, D):
    """test/twostage.jl:11-39 on seeded data: planted recovery, noiseless / noisy, k = 1, and l = k."""
    ok = 0
    for seed in range(8):
        A, x, b = cs.sparse_data(n=32, m=64, k=3, rng=100 + seed)
        y = cs.perturb(b, 5e-3, rng=seed)
        d = D(A)
        good = True
        for bb, l in ((b, 1), (y, 1), (b, 3), (y, 3)):
            xs = cs.srr(d, bb, 3, l=l)
            good &= np.array_equal(xs.nzind, x.nzind) and np.allclose(xs.nzval, x.nzval, atol=3e-2)
        x1 = cs.sparse_vector(64, 1, rng=seed)
        xs = cs.srr(d, A[:, x1.nzind] @ x1.nzval, 1)
        good &= np.array_equal(xs.nzind, x1.nzind) and np.allclose(xs.nzval, x1.nzval)
        ok += good
    assert ok >= 7


# ------------------------------------------------------------------------------------------------
# relevance matching pursuit and FoBa (src/stepwise.jl): loops over forward_step! / backward_step!
@pytest.mark.parametrize("cfg", [(32, 64, 3, 1e-2, np.float64), (128, 512, 10, 5e-2, np.float32), (96, 300, 8, 5e-2, np.float64),
                                 (256, 1500, 20, 5e-2, np.float32), (200, 150, 12, 5e-2, np.float64)])
def test_rmp_and_foba_match_oracle(cs, oracle, D, cfg):
    n, m, k, noise, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m, dtype=dtype)
    d = D(A)
    for seed in range(2):
        xs = cs.sparse_vector(m, k, rng=seed)
        y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, noise, rng=seed + 7)
        for name, fo, fg in (("rmp(delta)", lambda: oracle.rmp(A, y, noise), lambda: d.ctx.rmp(y, noise)),
                             ("rmp(delta,3)", lambda: oracle.rmp(A, y, noise, 3), lambda: d.ctx.rmp(y, noise, 3)),
                             ("foba", lambda: oracle.foba(A, y, noise), lambda: d.ctx.foba(y, noise)),
                             ("rmp(k)", lambda: oracle.rmp(A, y, k), lambda: d.ctx.rmp(y, k, kmax=min(n, m, 3 * k)))):
            if name == "rmp(k)" and min(n, m) > 3 * k:
                # rmp(A,b,k) first runs forward until the residual vanishes -- min(M,N) atoms on noisy data; with a
                # bounded support the library must refuse rather than truncate
                with pytest.raises(cs.CsmpError):
                    fg()
                continue
            ref, got = fo(), fg()
            assert np.array_equal(got[0], ref[0]), (name, seed, got[0], ref[0])
            assert close(got[1], ref[1], tight=False), name
    xg = cs.foba(d, y, noise)
    assert np.array_equal(xg.nzind, oracle.foba(A, y, noise)[0])


def test_rmp_foba_reference_known_answer(cs, D):
    """test/stepwise.jl:11-39 on seeded data (32 x 64, k = 3; rmp(A,b,k) fills all 32 rows before pruning)."""
    ok = 0
    for seed in range(8):
        A, x, b = cs.sparse_data(n=32, m=64, k=3, rng=300 + seed)
        y = cs.perturb(b, 1e-2, rng=seed)
        d = D(A)
        good = True
        for xs in (cs.rmp(d, y, 3), cs.rmp(d, y, 1e-2), cs.rmp(d, y, 1e-2, 3), cs.foba(d, b, 1e-2), cs.foba(d, y, 1e-2)):
            good &= np.array_equal(xs.nzind, x.nzind) and np.allclose(xs.nzval, x.nzval, atol=2e-2)
        ok += good
    assert ok >= 7


# ------------------------------------------------------------------------------------------------
# backward regression / LACE (src/backward.jl): all N <= M columns, then backward steps
@pytest.mark.parametrize("cfg", [(32, 32, 3, np.float64), (200, 150, 12, np.float32), (512, 300, 20, np.float32), (96, 96, 6, np.float64)])
def test_br_and_lace_match_oracle(cs, oracle, D, cfg):
    n, m, k, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + 3 * m, dtype=dtype)
    y = cs.perturb(b, 2e-2, rng=9)
    d = D(A)
    for lace in (False, True):
        for kw in (dict(k=k), dict(max_eps=0.03), dict(max_delta=0.01), dict(k=2 * k, max_eps=0.5)):
            ref = oracle.br(A, y, lace=lace, **kw)
            got = d.ctx.br(y, lace=lace, **kw)
            assert np.array_equal(got[0], ref[0]), (lace, kw, got[0], ref[0])
            assert close(got[1], ref[1], tight=False), (lace, kw)
    # public drivers, keyword and positional forms (src/backward.jl:27-41,148-162,226-242)
    ref = oracle.br(A, y, k=k)
    for f in (cs.br, cs.fbr):
        xg = f(d, y, sparsity=k)
        assert np.array_equal(xg.nzind, ref[0]) and close(xg.nzval, ref[1], tight=False)
    assert np.array_equal(cs.br(d, y, np.inf, np.inf, k).nzind, ref[0])
    assert np.array_equal(cs.lace(d, y, sparsity=k).nzind, oracle.br(A, y, k=k, lace=True)[0])
    with pytest.raises(ValueError):
        cs.br(np.zeros((4, 8)), np.zeros(4), sparsity=1)


def test_stepwise_family_edge_cases(cs, oracle, D):
    """Degenerate inputs through every §8f driver: b = 0, k = 1, fewer atoms than a wave, two rows."""
    rng = np.random.default_rng(5)
    # b = 0: forward steps stop at once (norm(r) > max_eps fails), the bulk initialisers still fill their support
    A, x, b = cs.sparse_data(n=40, m=30, k=3, rng=1)
    d = D(A)
    z = np.zeros(40)
    assert len(d.ctx.fr(z, 5)[0]) == 0 and len(oracle.fr(A, z, 5)[0]) == 0
    assert len(d.ctx.rmp(z, 1e-2)[0]) == 0 and len(d.ctx.foba(z, 1e-2)[0]) == 0 and len(d.ctx.rmp(z, 2)[0]) == 0
    got, ref = d.ctx.srr(z, 4), oracle.srr(A, z, 4)
    assert np.array_equal(got[0], ref[0]) and np.all(got[1] == 0.0) and got[2] == ref[2]
    got, ref = d.ctx.br(z, k=3), oracle.br(A, z, k=3)
    assert np.array_equal(got[0], ref[0]) and np.allclose(got[1], 0.0, atol=1e-300)
    # k = 1 everywhere
    y = cs.perturb(b, 1e-2, rng=2)
    for fo, fg in ((lambda: oracle.fr(A, y, 1), lambda: d.ctx.fr(y, 1)),
                   (lambda: oracle.srr(A, y, 1), lambda: d.ctx.srr(y, 1)),
                   (lambda: oracle.srr(A, y, 1, 1e-12, -1, 2, 1), lambda: d.ctx.srr(y, 1, 1e-12, -1, 2, 1)),
                   (lambda: oracle.rmp(A, y, 1), lambda: d.ctx.rmp(y, 1)),
                   (lambda: oracle.br(A, y, k=1), lambda: d.ctx.br(y, k=1)),
                   (lambda: oracle.ompr(A, y, 1, 1e-6), lambda: d.ctx.ompr(y, 1, 1e-6))):
        r, g = fo(), fg()
        assert np.array_equal(g[0], r[0]) and close(g[1], r[1], tight=False)
    # two rows, a handful of atoms (f32): every kernel runs with almost all lanes idle
    A2 = np.asfortranarray(rng.standard_normal((2, 7)).astype(np.float32))
    A2 /= np.linalg.norm(A2, axis=0)
    y2 = rng.standard_normal(2)
    d2 = D(A2)
    for fo, fg in ((lambda: oracle.fr(A2, y2, 2), lambda: d2.ctx.fr(y2, 2)),
                   (lambda: oracle.omp(A2, y2, 2, 0.0), lambda: d2.ctx.omp(y2, 2, 0.0)),
                   (lambda: oracle.srr(A2, y2, 1), lambda: d2.ctx.srr(y2, 1)),
                   (lambda: oracle.foba(A2, y2, 1e-3), lambda: d2.ctx.foba(y2, 1e-3))):
        r, g = fo(), fg()
        assert np.array_equal(g[0], r[0]), (g, r)
        assert close(g[1], r[1], tight=False)
    # argument errors mirror the reference's / the header's
    with pytest.raises(cs.CsmpError):
        d.ctx.srr(y, 0)
    with pytest.raises(cs.CsmpError):
        d.ctx.srr(y, 39, 1e-12, -1, 1, 2)  # k + l > M
    with pytest.raises(cs.CsmpError):
        d.ctx.srr(y, 3, 1e-12, -1, 3, 1)  # initialization 3 without the drawn atoms (csmp_srr_from takes them)
    with pytest.raises(cs.CsmpError):
        D(np.asfortranarray(rng.standard_normal((8, 20)))).ctx.br(np.zeros(8), k=1)  # underdetermined


def test_context_reuse_across_dictionaries_and_solver_families(cs, oracle):
    """One ctx, dictionaries of growing and shrinking size, every solver family in turn: the lazily
    allocated buffers (OLS rescaling, T = R^-1, panels, batch state) must follow the dictionary."""
    ctx = cs.Context(0)
    try:
        for (n, m, k, dtype, seed) in [(64, 200, 5, np.float64, 1), (256, 3000, 20, np.float32, 2), (48, 90, 4, np.float32, 3),
                                       (300, 280, 12, np.float64, 4)]:
            A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=seed, dtype=dtype)
            y = cs.perturb(b, 2e-2, rng=seed)
            ctx.set_dictionary(A)
            for got, ref in ((ctx.omp(y, k, 0.0), oracle.omp(A, y, k, 0.0)),
                             (ctx.fr(y, k), oracle.fr(A, y, k)),
                             (ctx.srr(y, k), oracle.srr(A, y, k)),
                             (ctx.ompr(y, k, 1e-9), oracle.ompr(A, y, k, 1e-9)),
                             (ctx.gomp(y, 2, k, 0.0), oracle.gomp(A, y, 2, k, 0.0)),
                             (ctx.foba(y, 2e-2), oracle.foba(A, y, 2e-2)),
                             (ctx.sp(y, k, 1e-12), oracle.sp(A, y, k, 1e-12))):
                assert np.array_equal(got[0], ref[0]), (n, m)
                assert close(got[1], ref[1], tight=False)
            if m <= n:
                got, ref = ctx.br(y, k=k), oracle.br(A, y, k=k)
                assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1], tight=False)
            B = np.asfortranarray(np.stack([y, 0.5 * y, -y], axis=1))
            idx, val, nnz = ctx.omp_batch_mfma(B, k, 0.0)
            ref = oracle.omp(A, y, k, 0.0)
            for s_ in range(3):
                assert np.array_equal(np.sort(idx[:nnz[s_], s_]), ref[0])
    finally:
        ctx.close()


@pytest.mark.parametrize("cfg", [(2048, 3000, 12, 7, np.float32), (4096, 2500, 10, 5, np.float32), (1024, 1500, 9, 4, np.float64),
                                 (130, 700, 8, 6, np.float32), (2048, 2000, 6, 2, np.float32)])
def test_fr_batch_matches_single_signal_calls(cs, oracle, D, cfg):
    """csmp_fr_batch (three signals per tick kernel where the sweep tiles exactly, one at a time otherwise) against
    the oracle and against csmp_fr, including per-signal stops at different steps."""
    n, m, k, nsig, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + nsig, dtype=dtype)
    d = D(A)
    rng = np.random.default_rng(nsig)
    cols = []
    for s_ in range(nsig):
        xs = cs.sparse_vector(m, max(1, k - (s_ % 3)), rng=rng)
        cols.append(cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 1e-2, rng=rng))
    B = np.asfortranarray(np.stack(cols, axis=1))
    for max_eps, min_delta in ((0.0, 0.0), (0.02, 0.0), (0.0, 0.05)):
        idx, val, nnz = d.ctx.fr_batch(B, k, max_eps, min_delta)
        for s_ in range(nsig):
            ref = oracle.fr(A, B[:, s_], k, max_eps, min_delta)
            one = d.ctx.fr(B[:, s_], k, max_eps, min_delta)
            assert nnz[s_] == len(ref[0]) and np.array_equal(idx[:nnz[s_], s_], ref[0]), (s_, max_eps, min_delta)
            assert close(val[:nnz[s_], s_], ref[1]) and np.array_equal(val[:nnz[s_], s_], one[1])  # bit-identical to csmp_fr
            assert np.all(idx[nnz[s_]:, s_] == -1)
    xs = cs.fr_batch(d, B, k)
    assert len(xs) == nsig and np.array_equal(xs[0].nzind, oracle.fr(A, B[:, 0], k)[0])


# ------------------------------------------------------------------------------------------ round 2
@pytest.mark.parametrize("kind", ["few_valued", "partial_dct", "one_magnitude", "common_component"])
def test_batched_mfma_structured_dictionaries(cs, oracle, kind):
    """The bf16 screen on dictionaries whose rounding errors are NOT independent: few-valued entries,
    partial-DCT rows, one magnitude per column (in bf16 each atom is scaled by its own factor), a strong common component.
    >= 200 signals per family, under both certificates (CSMP_OPT_BATCH_CERT): every support the batched path returns equals the
    exact path's -- a screen that would mislead shows up as `uncertain` (or `illcond`) and is re-solved, never silently -- and
    a sample is checked against the oracle."""
    M, N, nsig = 512, 4096, 200
    rng = np.random.default_rng(2026 + len(kind))
    A = cs.structured_dictionary(kind, M, N, rng=rng)
    A64 = A.astype(np.float64)
    d = cs.Dictionary(A)
    for family, k in (("pm1", 16), ("neartie", 2), ("neartie", 6)):
        B = np.empty((M, nsig), order="F")
        for s in range(nsig):
            sup = rng.choice(N, size=k, replace=False)
            x = rng.choice(np.array([-1.0, 1.0]), size=k)
            if family == "neartie":  # coefficients within 0.2 % of each other: exact correlations nearly tie
                x = x * (1.0 + 2e-3 * rng.random(k))
            B[:, s] = cs.perturb(A64[:, sup] @ x, 5e-3, rng=rng)
        i2, v2, n2 = d.ctx.omp_batch(B, k, EPS32)
        for screen, cert in ((DEFAULT_SCREEN, 1), (0, 0), (0, 1), (1, 0)):  # the defaults; bf16 statistical / rigorous; int8 statistical
            d.ctx.set_option("batch_screen", screen)
            d.ctx.set_option("batch_cert", cert)
            idx, val, nnz = d.ctx.omp_batch_mfma(B, k, EPS32)
            st = d.ctx.batch_stats()
            assert st["signals"] == nsig and st["resolved_exactly"] <= st["uncertain"] + st["illcond"]
            assert np.array_equal(nnz, n2), (kind, family, screen, cert)
            assert np.array_equal(idx, i2), (kind, family, screen, cert, int((idx != i2).any(axis=0).sum()))
            assert np.allclose(val, v2, rtol=1e-7, atol=1e-10)
        d.ctx.set_option("batch_cert", 1)
        d.ctx.set_option("batch_screen", DEFAULT_SCREEN)
        for s in range(0, nsig, 25):
            ref = oracle.omp(A, B[:, s], k, EPS32)
            assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]), (kind, family, s)
            assert close(val[:nnz[s], s], ref[1], tight=False)
    d.close()


def test_batched_mfma_resident_gram_option(cs, oracle, D):
    """CSMP_OPT_BATCH_GRAM: A_S'a from the resident G = A'A instead of a pass over the support's columns -- same supports, same
    coefficients (1e-9) as the default path and the oracle; switching the option off releases the matrix."""
    for dtype, shape in ((np.float32, (256, 2048, 12, 40)), (np.float64, (130, 700, 10, 33)), (np.float32, (1500, 3000, 16, 9))):
        n, m, k, nsig = shape
        A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m, dtype=dtype)
        d = D(A)
        rng = np.random.default_rng(nsig)
        B = np.asfortranarray(np.stack([cs.perturb(A.astype(np.float64) @ cs.sparse_vector(m, k, rng=rng).to_dense(), 5e-3, rng=rng)
                                        for _ in range(nsig)], axis=1))
        eps = float(np.finfo(dtype).eps)
        i0, v0, n0 = d.ctx.omp_batch_mfma(B, k, eps)
        d.ctx.set_option("batch_gram", 1)
        assert d.ctx.get_option("batch_gram") == 1
        i1, v1, n1 = d.ctx.omp_batch_mfma(B, k, eps)
        assert d.ctx.batch_stats()["illcond"] == 0
        d.ctx.set_option("batch_gram", 0)
        assert np.array_equal(i0, i1) and np.array_equal(n0, n1)
        assert np.allclose(v0, v1, rtol=1e-9, atol=1e-12)
        for s in range(0, nsig, 7):
            ref = oracle.omp(A, B[:, s], k, eps)
            assert np.array_equal(i1[:n1[s], s], ref[0]) and close(v1[:n1[s], s], ref[1])


def test_options_at_the_abi(cs, D):
    """csmp_set_option / csmp_get_option: defaults, range checks, unknown keys, inheritance by clones."""
    A, x, b = cs.sparse_data(n=64, m=256, k=4, rng=3, dtype=np.float32)
    d = D(A)
    c = d.ctx
    defaults = {"batch_cert": 1, "batch_gram": 0, "batch_window": 0, "pipeline": 1, "solves_in_flight": 3, "screened_sweep": 0,
                "batch_screen": DEFAULT_SCREEN}
    assert len(defaults) == len(cs._lib.OPTIONS) == 7
    for key, v in defaults.items():
        assert c.get_option(key) == v, key
    for key, bad in (("batch_cert", 2), ("batch_window", 129), ("pipeline", 2), ("batch_gram", -1), ("solves_in_flight", 5),
                     ("solves_in_flight", 0), ("screened_sweep", 4), ("batch_screen", 4)):
        with pytest.raises(cs.CsmpError):
            c.set_option(key, bad)
    for gone in (5, 6, 7, 8, 99):  # (5-8: keys of rounds 2-3 that no longer exist)
        with pytest.raises(cs.CsmpError):
            c.set_option(gone, 1)
    c.set_option("batch_cert", 0)
    c.set_option("solves_in_flight", 2)
    c.set_option("pipeline", 0)
    k2 = c.clone()
    assert k2.get_option("batch_cert") == 0 and k2.get_option("solves_in_flight") == 2 and k2.get_option("pipeline") == 0
    k2.close()
    for key, v in defaults.items():
        c.set_option(key, v)


def test_clone_keeps_the_dictionary_alive(cs, oracle):
    """a functor (a clone borrowing the parent's resident dictionary) must survive the parent's csmp_destroy and
    the parent's next csmp_set_dictionary -- the library-owned copy is reference counted."""
    A, x, b = cs.sparse_data(n=96, m=500, k=8, rng=5, dtype=np.float32)
    y = cs.perturb(b, 5e-3, rng=6)
    ref = oracle.omp(A, y, 8, EPS32)
    parent = cs.Context(0)
    parent.set_dictionary(A)
    child = parent.clone()
    A2, _, b2 = cs.sparse_data(n=80, m=300, k=5, rng=7, dtype=np.float64)
    parent.set_dictionary(A2)  # the clone still holds the first dictionary
    got = child.omp(y, 8, EPS32)
    assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
    ref2 = oracle.omp(A2, b2, 5, 1e-12)
    got2 = parent.omp(b2, 5, 1e-12)
    assert np.array_equal(got2[0], ref2[0])
    parent.close()  # ... and outlives the parent
    got = child.omp(y, 8, EPS32)
    assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
    child.close()


def test_lstsq_while_another_stream_saturates_the_gpu(cs, oracle):
    """the blocked Cholesky's row workgroups all read the unfactored diagonal block; with the GPU busy
    (another stream's large kernels) they start far apart, and a late one must not see workgroup 0's factored block.  The block
    now goes to a side buffer; run the whole-set least squares under load and compare with LAPACK."""
    import torch
    dev = torch.device("cuda", 0)
    A, x, b = cs.sparse_data(n=2048, m=4096, k=8, rng=11, dtype=np.float32)
    y = cs.perturb(b, 1e-2, rng=12)
    d = cs.Dictionary(A)
    big = torch.randn((8192, 8192), device=dev, dtype=torch.float32)
    side = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(13)
    for trial in range(6):
        n = int(rng.choice([200, 333, 512, 700, 1000]))
        cols = rng.choice(4096, size=n, replace=False)
        with torch.cuda.stream(side):
            for _ in range(12):
                big = torch.tanh(big @ big * 1e-4)
        coef = d.ctx.lstsq(cols, y)
        want = np.linalg.lstsq(A[:, cols].astype(np.float64), y, rcond=None)[0]
        assert np.allclose(coef, want, rtol=1e-8, atol=1e-10), (trial, n, np.abs(coef - want).max())
    torch.cuda.synchronize()
    d.close()


def test_full_size_config3_batched(cs, oracle):
    """BASELINE configs[2] at its real workload: 1024 signals sharing A 4096 x 65536 f32, k = 128, through
    csmp_omp_batch_mfma.  (i) oracle comparison on a sample: six signals x ALL 128 atoms, supports exact, coefficients 1e-6,
    under the library's defaults and under every certificate / screen / Gram option; (ii) every one of the 1024 supports and
    nnz equal to the exact single-signal path csmp_omp_batch, coefficients to 1e-9; (iii) the batch statistics."""
    import torch
    M, N, k, nsig = 4096, 65536, 128, 1024
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0xC0FFEE)
    At = torch.empty((N, M), dtype=torch.float32, device=dev)
    for lo in range(0, N, 8192):  # src/util.jl:21-27 recipe, cast once to Float32
        a = torch.randn((8192, M), generator=g, device=dev, dtype=torch.float64)
        a -= 1e-6 * a.mean(dim=1, keepdim=True)
        a /= a.norm(dim=1, keepdim=True)
        At[lo:lo + 8192] = a.to(torch.float32)
    d = cs.Dictionary(At)
    g2 = torch.Generator(device=dev).manual_seed(4242)
    B = torch.empty((nsig, M), dtype=torch.float64, device=dev)
    for lo in range(0, nsig, 64):  # planted +-1 k-sparse x0 + noise ||e|| = 5e-3 (src/util.jl:13-19,50-55)
        sel = torch.stack([torch.randperm(N, generator=g2, device=dev)[:k] for _ in range(64)])
        sign = torch.randint(0, 2, (64, k), generator=g2, device=dev).to(torch.float64) * 2 - 1
        b = torch.einsum("skm,sk->sm", At[sel].to(torch.float64), sign)
        e = torch.randn((64, M), generator=g2, device=dev, dtype=torch.float64)
        B[lo:lo + 64] = b + e * (5e-3 / e.norm(dim=1, keepdim=True))
    torch.cuda.synchronize()

    def run(fn, Bm, kk):
        n = Bm.shape[0]
        idx = torch.full((n, kk), -1, dtype=torch.int64, device=dev)
        val = torch.zeros((n, kk), dtype=torch.float64, device=dev)
        nnz = torch.zeros(n, dtype=torch.int64, device=dev)
        fn(Bm, kk, EPS32, idx, val, nnz)
        d.ctx.sync()
        return idx.cpu().numpy(), val.cpu().numpy(), nnz.cpu().numpy()

    # (i) the oracle, FULL k = 128 trajectories of six signals (tile edges of the 256-signal screening tiles and interior ones)
    A = np.asfortranarray(At.cpu().numpy().T)
    sample = [0, 255, 256, 511, 777, 1023]
    refs = {sgn: oracle.omp(A, B[sgn].cpu().numpy(), k, EPS32, nthreads=NT) for sgn in sample}

    def check_oracle(idx, val, nnz, what):
        for sgn in sample:
            ref = refs[sgn]
            assert nnz[sgn] == len(ref[0]) == k, (what, sgn)
            assert np.array_equal(idx[sgn], ref[0]), (what, sgn)
            assert close(val[sgn], ref[1], tight=False), (what, sgn)

    # (ii) the library's defaults: whole batch against the oracle sample and against the exact single-signal path
    idx, val, nnz = run(d.ctx.omp_batch_mfma_device, B, k)
    st = d.ctx.batch_stats()
    print("C3 defaults:", d.ctx.batch_screen_kernel(), st)
    check_oracle(idx, val, nnz, "defaults")
    i2, v2, n2 = run(d.ctx.omp_batch_device, B, k)
    check_oracle(i2, v2, n2, "csmp_omp_batch")
    assert np.array_equal(nnz, n2) and np.all(nnz == k)
    assert np.array_equal(idx, i2)
    assert np.allclose(val, v2, rtol=1e-9, atol=1e-12)
    # (iii) statistics: every signal accounted for, nothing ill-conditioned on a Gaussian dictionary, and the
    # certificate sends at most a handful of signals to the exact path
    assert st["signals"] == nsig and st["illcond"] == 0
    assert st["resolved_exactly"] == st["uncertain"] and st["uncertain"] <= 8, st
    # (iv) option combinations: certificate (0 statistical / 1 rigorous) x screen operands (3 binary16 / 0 bf16 / 1 int8) x resident Gram
    for cert, screen, gram in ((1, 3, 1), (1, 0, 0), (0, 3, 0), (0, 0, 0), (0, 1, 0), (0, 1, 1)):
        d.ctx.set_option("batch_cert", cert)
        d.ctx.set_option("batch_screen", screen)
        d.ctx.set_option("batch_gram", gram)
        oi, ov, on = run(d.ctx.omp_batch_mfma_device, B, k)
        sto = d.ctx.batch_stats()
        what = "cert %d screen %d gram %d" % (cert, screen, gram)
        print("C3", what, d.ctx.batch_screen_kernel(), sto)
        assert {0: "<bf16>", 1: "<i8>", 3: "<f16>"}[screen] in d.ctx.batch_screen_kernel(), what
        check_oracle(oi, ov, on, what)
        assert np.array_equal(on, n2) and np.array_equal(oi, i2), what
        assert np.allclose(ov, v2, rtol=1e-9, atol=1e-12), what
        assert sto["illcond"] == 0 and sto["uncertain"] <= 8, (what, sto)
    d.ctx.set_option("batch_gram", 0)
    d.close()


def test_step_level_mp_functor(cs, oracle, D):
    """MP(A, b) + update!(P, x) (src/matchingpursuit.jl:19-31) with the functor's DEFAULT capacity, at M = 4096: every
    step adds <a_i, r> to x[i] for the arg-max atom; the running x equals the oracle's mp after the same number of steps."""
    rng = np.random.default_rng(5)
    A = rng.standard_normal((4096, 6000)).astype(np.float32)
    A /= np.linalg.norm(A.astype(np.float64), axis=0).astype(np.float32)
    xs = cs.sparse_vector(6000, 6, rng=6)
    y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=7)
    d = D(A)
    P = cs.MP(d, y)  # default steps = 4096: needs no factorisation (and no LDS for one)
    x = cs.spzeros(6000)
    for t in range(1, 10):
        P(x)
        ref = oracle.mp(A, y, t)
        assert np.array_equal(x.nzind, ref[0]), (t, x.nzind, ref[0])
        assert np.allclose(x.nzval, ref[1], rtol=1e-6, atol=1e-12)
    P.close()


def test_functors_on_one_dictionary_are_independent(cs, oracle, D):
    """P1 = OMP(A, b1); P2 = OMP(A, b2) share A and nothing else (src/matchingpursuit.jl:44-60): interleaved updates, and a
    driver call on the same Dictionary in between, leave each object's factorisation alone."""
    A, x, b = cs.sparse_data(n=96, m=384, k=5, rng=31)
    y1 = cs.perturb(b, 5e-3, rng=32)
    y2 = cs.perturb(A @ cs.sparse_vector(384, 5, rng=33).to_dense(), 5e-3, rng=34)
    d = D(A)
    P1, P2 = cs.OMP(d, y1, 5), cs.OMP(d, y2, 5)
    x1, x2 = cs.spzeros(384), cs.spzeros(384)
    for t in range(5):
        P1(x1)
        if t == 2:
            cs.omp(d, y2, 3)  # a driver call on the shared Dictionary
            cs.sp(d, y1, 4)
        P2(x2)
    r1, r2 = oracle.omp(A, y1, 5, 0.0), oracle.omp(A, y2, 5, 0.0)
    assert np.array_equal(x1.nzind, r1[0]) and close(x1.nzval, r1[1])
    assert np.array_equal(x2.nzind, r2[0]) and close(x2.nzval, r2[1])
    P1.close()
    P2.close()


def test_reference_default_capacities_at_m4096(cs, oracle, D):
    """The reference's defaults size the QR by size(A,1): omp(A, b, eps) (k = M, src/matchingpursuit.jl:73), OMP(A, b)
    (:54) and GOMP(A, b, l) (:108) must work at the headline M = 4096 -- the append kernels' LDS follows the support
    actually built, not the capacity."""
    rng = np.random.default_rng(11)
    A = rng.standard_normal((4096, 5000)).astype(np.float32)
    A /= np.linalg.norm(A.astype(np.float64), axis=0).astype(np.float32)
    xs = cs.sparse_vector(5000, 5, rng=12)
    y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 1e-3, rng=13)
    d = D(A)
    got = cs.omp(d, y, 2e-3)  # k = size(A,1) = 4096; the residual test stops it
    ref = oracle.omp(A, y, 4096, 2e-3)
    assert np.array_equal(got.nzind, ref[0]) and close(got.nzval, ref[1]) and got.nnz == 5
    P = cs.OMP(d, y)
    xv = cs.spzeros(5000)
    for _ in range(5):
        P(xv)
    assert np.array_equal(xv.nzind, xs.nzind)
    P.close()
    G = cs.GOMP(d, y, 2)
    xg = cs.spzeros(5000)
    G(xg)
    assert xg.nnz == 2
    G.close()


@pytest.mark.parametrize("cfg", [(96, 400, 2, 7, 5, np.float32), (256, 2048, 4, 24, 9, np.float32), (130, 700, 3, 10, 4, np.float64)])
def test_gomp_batch_equals_single_calls(cs, oracle, D, cfg):
    """csmp_gomp_batch (two solves in flight on two streams, out of phase) = csmp_gomp signal by signal = the oracle, including
    the remainder step (k % l != 0), a residual stop on some signals, and an odd number of signals."""
    n, m, l, k, nsig, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + l, dtype=dtype)
    d = D(A)
    rng = np.random.default_rng(k)
    cols = []
    for s in range(nsig):
        kk = k if s % 3 else max(1, k // 2)  # every third signal is sparser: its residual test fires early
        cols.append(cs.perturb(A.astype(np.float64) @ cs.sparse_vector(m, kk, rng=rng).to_dense(), 1e-3, rng=rng))
    B = np.asfortranarray(np.stack(cols, axis=1))
    eps = 5e-3
    idx, val, nnz = d.ctx.gomp_batch(B, l, k, eps)
    for s in range(nsig):
        ref = oracle.gomp(A, B[:, s], l, k, eps)
        one = d.ctx.gomp(B[:, s], l, k, eps)
        assert nnz[s] == len(ref[0]) == len(one[0]), (s, nnz[s], len(ref[0]))
        assert np.array_equal(idx[:nnz[s], s], ref[0]) and np.array_equal(one[0], ref[0])
        assert close(val[:nnz[s], s], ref[1]) and np.array_equal(val[:nnz[s], s], one[1])
        assert np.all(idx[nnz[s]:, s] == -1)
    xs = cs.gomp_batch(d, B, l, k, eps)
    assert all(np.array_equal(xs[s].nzind, idx[:nnz[s], s]) for s in range(nsig))
    with pytest.raises(cs.CsmpError):
        d.ctx.gomp_batch(B, k + 1, k, eps)


@pytest.mark.parametrize("cfg", [(64, 256, 3, 5, np.float64), (640, 4096, 96, 7, np.float32)])
def test_sp_batch_equals_single_calls(cs, oracle, D, cfg):
    """csmp_sp_batch (several solves in flight, one context + host thread each) = csmp_sp signal by signal = the oracle; every
    in-flight count gives the same answer."""
    n, m, k, nsig, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + k, dtype=dtype)
    d = D(A)
    rng = np.random.default_rng(nsig)
    B = np.asfortranarray(np.stack([cs.perturb(A.astype(np.float64) @ cs.sparse_vector(m, k + (s % 3), rng=rng).to_dense(), 0.05 * (s % 2) + 5e-3, rng=rng)
                                    for s in range(nsig)], axis=1))
    first = None
    for flight in (3, 1, 2, 4):
        d.ctx.set_option("solves_in_flight", flight)
        idx, val, nnz, its = d.ctx.sp_batch(B, k, 1e-12)
        if first is None:
            first = (idx.copy(), val.copy(), nnz.copy(), its.copy())
            for s in range(nsig):
                ref = oracle.sp(A, B[:, s], k, 1e-12)
                one = d.ctx.sp(B[:, s], k, 1e-12)
                assert nnz[s] == len(ref[0]) == k and its[s] == ref[2] == one[2], (s, its[s], ref[2])
                assert np.array_equal(idx[:, s], ref[0]) and np.array_equal(idx[:, s], one[0])
                assert close(val[:, s], ref[1]) and np.allclose(val[:, s], one[1], rtol=1e-12, atol=0)
        else:
            assert np.array_equal(idx, first[0]) and np.array_equal(nnz, first[2]) and np.array_equal(its, first[3])
            assert np.allclose(val, first[1], rtol=1e-12, atol=0)
    d.ctx.set_option("solves_in_flight", 3)
    xs = cs.sp_batch(d, B, k)
    assert all(np.array_equal(xs[s].nzind, first[0][:, s]) for s in range(nsig))


def test_batch_forms_edge_cases(cs, oracle, D):
    """Empty and tiny batches, k = 1, l = k, ragged shapes (M = 37, N = 301: nothing is a multiple of a tile), one signal, more
    solves in flight than signals -- through csmp_gomp_batch, csmp_sp_batch and csmp_omp_batch_mfma with the Gram option."""
    A, x, b = cs.sparse_data(n=37, m=301, k=3, rng=2, dtype=np.float64)
    d = D(A)
    rng = np.random.default_rng(9)
    B = np.asfortranarray(np.stack([cs.perturb(A @ cs.sparse_vector(301, 3, rng=rng).to_dense(), 1e-3, rng=rng) for _ in range(3)], axis=1))
    E = np.zeros((37, 0), order="F")
    for fn in (lambda: d.ctx.gomp_batch(E, 1, 2, 1e-9), lambda: d.ctx.sp_batch(E, 2, 1e-9)):
        out = fn()
        assert out[0].shape[1] == 0 and len(out[2]) == 0
    for l, k in ((1, 1), (3, 3), (2, 5)):
        idx, val, nnz = d.ctx.gomp_batch(B, l, k, 1e-9)
        for s in range(3):
            ref = oracle.gomp(A, B[:, s], l, k, 1e-9)
            assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]) and close(val[:nnz[s], s], ref[1])
    one = B[:, :1].copy(order="F")
    d.ctx.set_option("solves_in_flight", 4)
    idx, val, nnz, its = d.ctx.sp_batch(one, 3, 1e-12)
    ref = oracle.sp(A, one[:, 0], 3, 1e-12)
    assert nnz[0] == 3 and np.array_equal(idx[:, 0], ref[0]) and close(val[:, 0], ref[1]) and its[0] == ref[2]
    d.ctx.set_option("solves_in_flight", 3)
    d.ctx.set_option("batch_gram", 1)
    for k in (1, 4):
        idx, val, nnz = d.ctx.omp_batch_mfma(B, k, 1e-9)
        for s in range(3):
            ref = oracle.omp(A, B[:, s], k, 1e-9)
            assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]) and close(val[:nnz[s], s], ref[1])
    d.ctx.set_option("batch_gram", 0)
    with pytest.raises(cs.CsmpError):
        d.ctx.sp_batch(B, 19, 1e-9)  # 2k > M: the reference's error(...) (src/twostage.jl:55)


def test_solve_in_flight_with_clones(cs, oracle, D):
    """solve_in_flight: ompr / srr / fr for many signals, three at a time on clones driven by host threads, equal the one-at-a-time
    calls and the oracle."""
    n, m, k, nsig = 96, 600, 6, 7
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=31, dtype=np.float32)
    d = D(A)
    rng = np.random.default_rng(32)
    cols = [cs.perturb(A.astype(np.float64) @ cs.sparse_vector(m, k + 2, rng=rng).to_dense(), 0.05, rng=rng) for _ in range(nsig)]
    got = cs.solve_in_flight(d, cols, lambda c, y: c.ompr(y, k, 1e-6), in_flight=3)
    for s in range(nsig):
        ref = oracle.ompr(A, cols[s], k, 1e-6)
        assert np.array_equal(got[s][0], ref[0]) and close(got[s][1], ref[1]) and got[s][2] == ref[2]
    got = cs.solve_in_flight(d, cols, lambda c, y: c.srr(y, k), in_flight=2)
    for s in range(nsig):
        ref = oracle.srr(A, cols[s], k)
        assert np.array_equal(got[s][0], ref[0]) and close(got[s][1], ref[1])
    with pytest.raises(cs.CsmpError):  # an error inside a worker surfaces
        cs.solve_in_flight(d, cols, lambda c, y: c.sp(y, n, 1e-6), in_flight=3)


def test_reference_default_capacity_reaches_size_a1(cs, oracle, D):
    """The reference's only bound on a support is size(A,1): omp(A, b, 0.0) / OMP(A, b) default to k = size(A,1)
    (src/matchingpursuit.jl:54,89) and update! runs until nnz(x) == size(A,1) (:63).  At M = 4096 the append kernels' five
    support-length LDS vectors hold ~3900 columns; beyond that the same kernel bodies run with those vectors in global memory
    (k_qr1s / k_qr2s / k_qr3s), so a signal no stopping rule ends gets its FULL 4096-atom support -- every selection, the support
    and the coefficients against the oracle.  (Rounds 2-3 stopped at ~3900 with CSMP_WCAPACITY.)"""
    lib = cs._lib
    rng = np.random.default_rng(41)
    M, N = 4096, 4608
    A = rng.standard_normal((M, N)).astype(np.float32)
    A /= np.linalg.norm(A.astype(np.float64), axis=0).astype(np.float32)
    y = rng.standard_normal(M)  # dense in every atom: the residual never reaches 0 before the support is full
    d = D(A)
    idx, val, order = d.ctx.omp(y, M, 0.0)
    assert d.ctx.last_status == lib.OK
    assert len(idx) == M and len(set(idx.tolist())) == M
    ref = oracle.omp(A, y, M, 0.0, nthreads=NT)
    assert len(ref[0]) == M
    assert np.array_equal(order, ref[2]) and np.array_equal(idx, ref[0])
    assert np.allclose(val, ref[1], rtol=1e-6, atol=1e-6 * np.abs(ref[1]).max())  # (a square 4096 x 4096 system: cond ~ 1e4)
    r = y - A[:, idx].astype(np.float64) @ val
    assert np.linalg.norm(r) < 1e-8 * np.linalg.norm(y)  # a full support reproduces b
    # a smaller request on the same context is unaffected
    i2, v2, o2 = d.ctx.omp(y, 48, 0.0)
    assert d.ctx.last_status == lib.OK and np.array_equal(o2, ref[2][:48])
    # the wrapper's default form, omp(A, b, eps) with k = size(A,1), and the functor's default capacity
    xv = cs.omp(d, y, 0.0)
    assert xv.nnz == M and np.array_equal(xv.nzind, ref[0])
    # batch form: beyond the LDS kernels' capacity the signals go one at a time through the same chain
    B = np.asfortranarray(np.stack([y, -y], axis=1))
    bi, bv, bn = d.ctx.omp_batch(B, M, 0.0)
    assert d.ctx.last_status == lib.OK and bn[0] == M and bn[1] == M
    assert np.array_equal(bi[:, 0], ref[0]) and np.array_equal(bi[:, 1], ref[0])
    assert np.allclose(bv[:, 0], ref[1], rtol=1e-6, atol=1e-6 * np.abs(ref[1]).max()) and np.allclose(bv[:, 1], -bv[:, 0], rtol=1e-9, atol=1e-12)
    # gomp(A, b, l) at its default capacity size(A,1) (:108): l = 3 does not divide 4096, the remainder step fills the support
    gi, gv, go = d.ctx.gomp(y, 3, M, 0.0)
    rg = oracle.gomp(A, y, 3, M, 0.0, nthreads=NT)
    assert len(gi) == len(rg[0]) == M and np.array_equal(go, rg[2])
    assert np.linalg.norm(y - A[:, gi].astype(np.float64) @ gv) < 1e-8 * np.linalg.norm(y)


def test_capacity_growth_does_not_disable_the_removal_solvers(cs, oracle, D):
    """A call that grows the solver slot past 1023 columns (sp with 2k = 1024) must not make every later
    srr / ompr / rmp / foba / solver_remove on the same Dictionary fail: the slot is rebuilt at the size they need."""
    A, x, b = cs.sparse_data(n=1100, m=3000, k=6, rng=41, dtype=np.float32)
    y = cs.perturb(b, 5e-3, rng=42)
    d = D(A)
    big = cs.sp(d, y, 512)  # capacity 1024
    assert big.nnz == 512
    for name, call, ref in [("srr", lambda: cs.srr(d, y, 6), lambda: oracle.srr(A, y, 6)),
                            ("ompr", lambda: cs.ompr(d, y, 6, 1e-6), lambda: oracle.ompr(A, y, 6, 1e-6))]:
        got = call()
        r = ref()
        assert np.array_equal(got.nzind, r[0]), name
        assert close(got.nzval, r[1], tight=False), name
    # ... and the other way round: the small slot grows again for the next large request
    again = cs.sp(d, y, 512)
    assert np.array_equal(again.nzind, big.nzind) and np.array_equal(again.nzval, big.nzval)


def _colsharded(cs, A, y, k, eps, cuts):
    """omp_colsharded over virtual ranks: one context per column block [cuts[i], cuts[i+1])."""
    import torch
    ctxs, shards = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        c = cs.Context(0)
        c.set_dictionary(np.asfortranarray(A[:, lo:hi]))
        ctxs.append(c)
        shards.append(cs.HipColumnShard(c, lo, torch.device("cuda", 0)))
    try:
        return cs.omp_colsharded(shards, y, k, eps)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("cfg", [(256, 1024, 24, np.float32, (0, 512, 1024)), (130, 701, 12, np.float64, (0, 233, 467, 701)),
                                 (4096, 3000, 20, np.float32, (0, 1000, 3000))])
def test_column_sharded_omp_equals_omp(cs, oracle, D, cfg):
    """one signal, columns sharded over (virtual) ranks -- per step every rank sweeps its slice, one
    record per rank is exchanged, every rank appends the winner.  Selection order, support and coefficients must be
    those of csmp_omp on the whole dictionary (bitwise: the same kernels see the same numbers) and of the oracle."""
    n, m, k, dtype, cuts = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m, dtype=dtype)
    y = cs.perturb(b, 5e-3, rng=3)
    eps = float(np.finfo(dtype).eps)
    idx, val, order = _colsharded(cs, A, y, k, eps, cuts)
    d = D(A)
    full = d.ctx.omp(y, k, eps)
    assert np.array_equal(order, full[2]) and np.array_equal(idx, full[0]) and np.array_equal(val, full[1])
    ref = oracle.omp(A, y, k, eps)
    assert np.array_equal(order, ref[2]) and np.array_equal(idx, ref[0]) and close(val, ref[1])


def test_column_sharded_omp_ties_and_stops(cs, oracle):
    """Ties across shards go to the LOWER global index (Julia argmax over the whole dictionary, src/matchingpursuit.jl:184):
    one planted atom exists in both shards.  The driver's residual test (:79) stops every rank at the same step."""
    A, x, b = cs.sparse_data(n=64, m=200, k=4, rng=9)
    A = A.copy()
    j0 = int(x.nzind[0])
    dup = 150 if j0 < 100 else 20
    assert dup not in x.nzind
    A[:, dup] = A[:, j0]  # the same atom in the other shard
    y = A @ x.to_dense()
    for k, eps in [(4, 0.0), (8, 1e-9)]:
        got = _colsharded(cs, A, y, k, eps, (0, 100, 200))
        ref = oracle.omp(A, y, k, eps)
        assert np.array_equal(got[2], ref[2]), (got[2], ref[2])
        assert np.array_equal(got[0], ref[0]) and close(got[1], ref[1])
        assert max(j0, dup) not in got[0] and min(j0, dup) in got[0]


@pytest.mark.parametrize("workload", ["omp", "colsharded", "batched", "batched8", "omp_rccl_world1"])
def test_bench_two_ranks_rehearsal_on_one_gpu(workload, tmp_path):
    """The N > 1 code of bench.py end to end on the GPU box: two ranks under torchrun sharing the one GPU (--share-gpu: the
    exchange over gloo, because RCCL refuses two ranks on one device).  Checks the JSON contract of the multi-rank line (the compact
    headline on stdout, the detail in bench_secondary.json; both --full): ranks seen, the gathered rows and the recomputation check of the
    signal-sharded workload, the cross-rank agreement of the column-sharded one.  omp_rccl_world1: ONE rank under the launcher
    with the "nccl" backend -- the path the driver's N > 1 runs take, with the collective inside the library (csmp_omp_sharded).
    Not a scaling measurement."""
    import json
    import subprocess
    import sys
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))  # a free rendezvous port
    port = sk.getsockname()[1]
    sk.close()
    world = 8 if workload == "batched8" else 1 if workload == "omp_rccl_world1" else 2  # batched8 = BASELINE configs[3] in shape: 8192 signals over 8 ranks
    extra = {"omp": ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-secondary"],
             "omp_rccl_world1": ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-secondary"],
             "colsharded": ["--workload", "colsharded", "--steps", "1", "--warmup", "0"],
             "batched": ["--workload", "batched", "--steps", "1", "--warmup", "0"],
             "batched8": ["--workload", "batched", "--steps", "1", "--warmup", "0"]}[workload]
    share = [] if workload == "omp_rccl_world1" else ["--share-gpu"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--full"] + share + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    last = out.stdout.strip().splitlines()[-1]
    assert len(last) < 4096
    line = json.loads(last)  # the compact headline IS the last stdout line
    detail = json.load(open(tmp_path / "bench_secondary.json"))
    assert line["n_gpus"] == world and line["ranks_seen"] == world and len(line["devices"]) == world and "error" not in line
    assert abs(line["value"] - detail["value"]) <= 1e-5 * detail["value"]
    if workload in ("omp", "omp_rccl_world1"):
        assert detail["gathered_rows"] == world * 2 and line["gather_check"]["rows_ok"]
        assert line["gather_check"]["first_signal_of_every_rank_equals_rank0_recomputation"] == [True] * world
        assert detail["atoms_selected"] == world * 2 * 256
        assert line["config"]["collective"] == ("ncclAllGather inside csmp_omp_sharded" if workload == "omp_rccl_world1" else "torch.distributed all_gather")
    elif workload == "colsharded":
        assert line["ranks_agree_on_first_support"] and detail["supports_gathered"] == 2 and line["scaling"] == "strong"
    else:
        assert line["matches_exact_path_on_sample"] and abs(line["value"] * line["ms_per_step"] * 1e-3 - world * 1024 * 128) < 5.0


def test_bench_plain_run_and_dumped_outputs(cs, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times K steps and prints the headline only (no CPU baseline, no secondary
    workloads, no detail file); --dump-outputs writes what the last timed step returned, and that is a lone omp call's result on
    the same signal (signal W + K - 1 of rank 0)."""
    import json
    import subprocess
    import sys
    import torch
    import bench
    K, W = 2, 1
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                          "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == K and line["warmup"] == W and line["ms_per_step"] > 0 and line["unit"] == "atoms/s"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 256) < 1.0  # (every solve selects k = 256 atoms here)
    assert "cpu_baseline" not in line and "secondary" not in line and not (tmp_path / bench.DETAIL_FILE).exists()
    got = {n: np.load(tmp_path / "dump" / (n + ".npy")) for n in ("idx", "val", "nnz")}
    assert all(a.dtype == np.float64 for a in got.values())
    dev = torch.device("cuda", 0)
    At = bench.make_dictionary(torch, dev)
    b = bench.make_signals(torch, dev, At, 0, K + W)[K + W - 1].cpu().numpy()
    d = cs.Dictionary(At, device=0)
    try:
        i, v, o = d.ctx.omp(b, 256, EPS32)
    finally:
        d.close()
    n = int(got["nnz"][0])
    gi, gv = got["idx"][:n], got["val"][:n]
    pg, pr = np.argsort(gi), np.argsort(i)  # (the same support and coefficients, whichever order each call lists them in)
    assert n == len(i) and np.array_equal(gi[pg], i[pr]) and close(gv[pg], v[pr], tight=False)


# ------------------------------------------------------------------ screened single-signal sweep (CSMP_OPT_SCREENED_SWEEP)
@pytest.mark.parametrize("shape", [(64, 256, 6), (50, 301, 5), (130, 700, 10), (512, 4096, 24), (1500, 3000, 16), (4096, 2500, 12), (37, 5, 3)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_screened_sweep_omp_matches_oracle(cs, oracle, D, shape, dtype):
    """csmp_omp with the sweep over the bf16 image (k_sweep_bf16 + k_pick1, certified picks): supports, selection order and
    coefficients of the oracle (src/matchingpursuit.jl:62-90), under both certificates; the counters say the screened path ran."""
    n, m, k = shape
    A, x, b = cs.sparse_data(n=n, m=m, k=min(k, m), rng=n + m + k, dtype=dtype)
    eps = float(np.finfo(dtype).eps)
    d = D(A)
    d.ctx.screened_stats(reset=True)
    for image, cert in ((3, 1), (3, 0), (1, 0), (1, 1), (2, 0)):  # binary16 and bf16 images under both certificates, int8 image (statistical only)
        d.ctx.set_option("screened_sweep", image)
        d.ctx.set_option("batch_cert", cert)
        for seed, noise in ((0, 0.0), (1, 5e-3), (2, 1e-1)):
            y = cs.perturb(b, noise, rng=seed) if noise else b
            ref = oracle.omp(A, y, k, eps)
            got = d.ctx.omp(y, k, eps)
            assert np.array_equal(got[0], ref[0]), (image, cert, seed, got[0], ref[0])
            assert np.array_equal(got[2], ref[2]), "selection order"
            assert close(got[1], ref[1], tight=False)
    st = d.ctx.screened_stats()
    assert st["solves"] == 15 and 0 <= st["fallbacks"] <= 15
    d.ctx.set_option("batch_cert", 1)
    d.ctx.set_option("screened_sweep", 0)
    d.ctx.omp(b, k, eps)
    assert d.ctx.screened_stats()["solves"] == 15, "option off: the exact sweep"


def test_screened_sweep_certifies_on_gaussian_dictionaries(cs, oracle, D):
    """On the benchmark's kind of dictionary the statistical certificate has to hold at (nearly) every step -- a screened
    path that always falls back would be correct and useless."""
    A, x, b = cs.sparse_data(n=1024, m=8192, k=24, rng=77, dtype=np.float32)
    d = D(A)
    for image in (3, 1, 2):  # binary16 under the RIGOROUS certificate (the default); bf16 / int8 under the statistical one
        d.ctx.set_option("batch_cert", 1 if image == 3 else 0)
        d.ctx.set_option("screened_sweep", image)
        d.ctx.screened_stats(reset=True)
        rng = np.random.default_rng(4)
        for s in range(8):
            sup = rng.choice(8192, size=24, replace=False)
            y = cs.perturb(A[:, sup].astype(np.float64) @ rng.choice(np.array([-1.0, 1.0]), size=24), 5e-3, rng=rng)
            ref = oracle.omp(A, y, 24, EPS32)
            got = d.ctx.omp(y, 24, EPS32)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and close(got[1], ref[1], tight=False)
        st = d.ctx.screened_stats()
        assert st["solves"] == 8 and st["fallbacks"] <= 1, (image, st)
    d.ctx.set_option("screened_sweep", 0)


@pytest.mark.parametrize("kind", ["few_valued", "partial_dct", "one_magnitude", "common_component"])
def test_screened_sweep_structured_dictionaries(cs, oracle, kind):
    """Dictionaries whose bf16 rounding errors are not independent: whatever the certificate decides, the result is the exact
    path's (an uncertified step repeats the solve with the exact sweep)."""
    M, N, nsig = 512, 4096, 24
    rng = np.random.default_rng(99 + len(kind))
    A = cs.structured_dictionary(kind, M, N, rng=rng)
    A64 = A.astype(np.float64)
    d = cs.Dictionary(A)
    for family, k in (("pm1", 16), ("neartie", 4)):
        B = np.empty((M, nsig), order="F")
        for s in range(nsig):
            sup = rng.choice(N, size=k, replace=False)
            x = rng.choice(np.array([-1.0, 1.0]), size=k)
            if family == "neartie":
                x = x * (1.0 + 2e-3 * rng.random(k))
            B[:, s] = cs.perturb(A64[:, sup] @ x, 5e-3, rng=rng)
        d.ctx.set_option("screened_sweep", 0)
        i2, v2, n2 = d.ctx.omp_batch(B, k, EPS32)
        for image, cert in ((3, 1), (3, 0), (1, 0), (1, 1), (2, 0)):
            d.ctx.set_option("screened_sweep", image)
            d.ctx.set_option("batch_cert", cert)
            idx, val, nnz = d.ctx.omp_batch(B, k, EPS32)  # two screened solves in flight
            assert np.array_equal(nnz, n2) and np.array_equal(idx, i2), (kind, family, cert)
            assert np.allclose(val, v2, rtol=1e-7, atol=1e-10)
            for s in range(0, nsig, 8):
                got = d.ctx.omp(B[:, s], k, EPS32)
                assert np.array_equal(got[0], np.sort(i2[:n2[s], s])) or np.array_equal(got[0], i2[:n2[s], s])
        d.ctx.set_option("batch_cert", 0)
        for s in range(0, nsig, 6):
            ref = oracle.omp(A, B[:, s], k, EPS32)
            assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]), (kind, family, s)
    d.close()


def test_screened_sweep_ties_stops_and_fallback(cs, oracle, D):
    """Duplicate atoms (the certificate cannot separate them: the solve falls back and the lowest index wins, as findmax does),
    the residual test, a support that fills up, a zero signal, more duplicates than a sweep workgroup lists."""
    rng = np.random.default_rng(12)
    A = rng.standard_normal((96, 700)).astype(np.float32)
    A /= np.linalg.norm(A, axis=0)
    for c in (250, 251, 252, 253, 254, 699):  # six exact copies of atom 17, five of them in ONE sweep workgroup's columns
        A[:, c] = A[:, 17]
    A = np.asfortranarray(A)
    d = D(A)
    d.ctx.set_option("screened_sweep", 1)
    d.ctx.screened_stats(reset=True)
    y = 3.0 * A[:, 17].astype(np.float64) + 0.5 * A[:, 400].astype(np.float64) - 0.25 * A[:, 5].astype(np.float64)
    ref = oracle.omp(A, y, 3, EPS32)
    got = d.ctx.omp(y, 3, EPS32)
    assert got[2][0] == 17 and np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    assert d.ctx.screened_stats()["fallbacks"] <= 1  # (copies inside the rescoring window tie exactly: lowest index, certified)
    # more copies than the sweep's workgroups list (4 each) or the window holds: the certificate has to fail, the exact sweep decides
    A2 = rng.standard_normal((96, 3000)).astype(np.float32)
    A2 /= np.linalg.norm(A2, axis=0)
    A2[:, :1500] = A2[:, [7]]
    A2 = np.asfortranarray(A2)
    d2 = D(A2)
    d2.ctx.set_option("screened_sweep", 1)
    d2.ctx.screened_stats(reset=True)
    yd = 2.0 * A2[:, 7].astype(np.float64) + 0.7 * A2[:, 2500].astype(np.float64)
    ref = oracle.omp(A2, yd, 2, EPS32)
    got = d2.ctx.omp(yd, 2, EPS32)
    assert got[2][0] == 0 and np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    assert d2.ctx.screened_stats() == {"solves": 1, "fallbacks": 1}
    # eps-stop: exact 2-sparse signal, k = 10
    y2 = 2.0 * A[:, 100].astype(np.float64) - A[:, 600].astype(np.float64)
    ref = oracle.omp(A, y2, 10, 1e-6)
    got = d.ctx.omp(y2, 10, 1e-6)
    assert np.array_equal(got[0], ref[0]) and len(got[0]) == 2 and close(got[1], ref[1], tight=False)
    # zero signal: the reference adds atom 1 (findmax of zeros) then stops on the residual test
    ref = oracle.omp(A, np.zeros(96), 4, EPS32)
    got = d.ctx.omp(np.zeros(96), 4, EPS32)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    # batch form: every kind of signal side by side, odd count
    B = np.asfortranarray(np.stack([y, y2, np.zeros(96), -y, y2 + y], axis=1))
    idx, val, nnz = d.ctx.omp_batch(B, 6, 1e-6)
    for s in range(5):
        ref = oracle.omp(A, B[:, s], 6, 1e-6)
        assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]), s
        if len(ref[1]) and np.all(np.isfinite(ref[1])):
            assert close(val[:nnz[s], s], ref[1], tight=False)
    d.ctx.set_option("screened_sweep", 0)


def test_screened_sweep_full_size_config2(cs, oracle):
    """BASELINE configs[1] (4096 x 65536 f32, k = 256) with the screened sweep: the complete solve equals the exact path's
    (support, order, coefficients), an oracle prefix pins both; the certificate holds throughout (no fallback)."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    At = bench.make_dictionary(torch, dev)
    B = bench.make_signals(torch, dev, At, 500, 2)
    d = cs.Dictionary(At, device=0)
    y = B[0].cpu().numpy()
    exact = d.ctx.omp(y, 256, EPS32)
    # the int8 and bf16 images under the statistical certificate, then the binary16 image under the RIGOROUS one (the library's default
    # certificate; the rest of the test keeps it): the provable mode has to certify here too, or it would be correct and useless
    for image, cert in ((2, 0), (1, 0), (3, 1)):
        d.ctx.set_option("batch_cert", cert)
        d.ctx.set_option("screened_sweep", image)
        d.ctx.screened_stats(reset=True)
        got = d.ctx.omp(y, 256, EPS32)
        assert np.array_equal(got[0], exact[0]) and np.array_equal(got[2], exact[2]), image
        assert np.allclose(got[1], exact[1], rtol=1e-9, atol=1e-12)
        st = d.ctx.screened_stats()
        # (the column groups are handed out dynamically: which workgroup lists which atoms varies from run to run, and with it -- very
        # rarely -- whether a pick certifies; the results above do not depend on it)
        assert st["solves"] == 1 and st["fallbacks"] <= 1, (image, cert, st)
        print("C2 screened image", image, "cert", cert, st)
    A = np.asfortranarray(At.cpu().numpy().T)
    ref = oracle.omp(A, y, 12, EPS32)
    assert np.array_equal(got[2][:12], ref[2])
    idx = torch.full((2, 256), -1, dtype=torch.int64, device=dev)
    val = torch.zeros((2, 256), dtype=torch.float64, device=dev)
    nnz = torch.zeros(2, dtype=torch.int64, device=dev)
    d.ctx.omp_batch_device(B, 256, EPS32, idx, val, nnz)
    d.ctx.sync()
    assert int(nnz[0]) == len(exact[0]) and np.array_equal(np.sort(idx[0, :int(nnz[0])].cpu().numpy()), np.sort(exact[0]))
    d.close()


@pytest.mark.parametrize("shape", [(32, 48, 3, 2), (64, 256, 9, 4), (37, 101, 7, 3), (256, 1024, 32, 4), (300, 5000, 40, 16), (512, 4096, 24, 4),
                                   (1500, 3000, 17, 4)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_screened_sweep_gomp_matches_oracle(cs, oracle, D, shape, dtype):
    """csmp_gomp / csmp_gomp_batch with the screened sweep (k_sweep_bf16 + k_pickS: the top-l pick certified as a whole):
    supports, INSERTION ORDER and coefficients of the oracle (src/matchingpursuit.jl:116-148), both certificates, l from 2 to 16,
    k not a multiple of l (the remainder step)."""
    n, m, k, l = shape
    eps = float(np.finfo(dtype).eps)
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n * 17 + m, dtype=dtype)
    d = D(A)
    d.ctx.set_option("screened_sweep", 1)
    d.ctx.screened_stats(reset=True)
    ys = []
    for seed in range(3):
        xs = cs.sparse_vector(m, k, rng=seed)
        ys.append(cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3 if seed else 0.0, rng=seed + 50) if seed else A[:, xs.nzind].astype(np.float64) @ xs.nzval)
    refs = [oracle.gomp(A, y, l, k, eps) for y in ys]
    for image, cert in ((3, 1), (3, 0), (1, 0), (1, 1), (2, 0)):
        d.ctx.set_option("screened_sweep", image)
        d.ctx.set_option("batch_cert", cert)
        for y, ref in zip(ys, refs):
            got = d.ctx.gomp(y, l, k, eps)
            assert np.array_equal(got[2], ref[2]), ("insertion order", cert)
            assert np.array_equal(got[0], ref[0])
            if np.all(np.isfinite(ref[1])):
                assert close(got[1], ref[1], tight=False)
        idx, val, nnz = d.ctx.gomp_batch(np.asfortranarray(np.stack(ys, axis=1)), l, k, eps)
        for s, ref in enumerate(refs):
            assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]), (cert, s)
    st = d.ctx.screened_stats()
    assert st["solves"] == 30 and st["fallbacks"] <= 30
    d.ctx.set_option("batch_cert", 1)
    d.ctx.set_option("screened_sweep", 0)


@pytest.mark.parametrize("kind", ["few_valued", "partial_dct", "one_magnitude", "common_component"])
def test_screened_sweep_gomp_structured_dictionaries(cs, oracle, kind):
    M, N, nsig, k, l = 512, 4096, 12, 16, 4
    rng = np.random.default_rng(7 + len(kind))
    A = cs.structured_dictionary(kind, M, N, rng=rng)
    A64 = A.astype(np.float64)
    d = cs.Dictionary(A)
    B = np.empty((M, nsig), order="F")
    for s in range(nsig):
        sup = rng.choice(N, size=k, replace=False)
        x = rng.choice(np.array([-1.0, 1.0]), size=k) * (1.0 + (2e-3 * rng.random(k) if s % 2 else 0.0))
        B[:, s] = cs.perturb(A64[:, sup] @ x, 5e-3, rng=rng)
    i2, v2, n2 = d.ctx.gomp_batch(B, l, k, EPS32)
    for image, cert in ((3, 1), (3, 0), (1, 0), (1, 1), (2, 0)):
        d.ctx.set_option("screened_sweep", image)
        d.ctx.set_option("batch_cert", cert)
        idx, val, nnz = d.ctx.gomp_batch(B, l, k, EPS32)
        assert np.array_equal(nnz, n2) and np.array_equal(idx, i2), (kind, cert)
        assert np.allclose(val, v2, rtol=1e-7, atol=1e-10)
    for s in range(0, nsig, 4):
        ref = oracle.gomp(A, B[:, s], l, k, EPS32)
        got = d.ctx.gomp(B[:, s], l, k, EPS32)
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0])
    d.close()


def test_screened_sweep_gomp_duplicates_and_small_dictionaries(cs, oracle, D):
    """Exact copies among the top-l (GOMP takes an atom AND its copy: the reference's least squares is singular there, only the
    support is defined), fewer atoms than l, a dictionary of one sweep workgroup."""
    rng = np.random.default_rng(3)
    A = rng.standard_normal((64, 300)).astype(np.float32)
    A /= np.linalg.norm(A, axis=0)
    A[:, 250] = A[:, 17]
    A = np.asfortranarray(A)
    d = D(A)
    d.ctx.set_option("screened_sweep", 1)
    y = 3.0 * A[:, 17].astype(np.float64) + 0.5 * A[:, 40].astype(np.float64)
    ref = oracle.gomp(A, y, 2, 4, EPS32)  # (the reference's coefficients are +-Inf from here on and it stops; only the first step is defined)
    got = d.ctx.gomp(y, 2, 4, EPS32)
    d.ctx.set_option("screened_sweep", 0)
    exact = d.ctx.gomp(y, 2, 4, EPS32)
    assert np.array_equal(got[2][:2], ref[2][:2]) and np.array_equal(got[2], exact[2]) and np.array_equal(got[0], exact[0])
    A3 = np.asfortranarray(rng.standard_normal((16, 3)))
    d3 = D(A3)
    d3.ctx.set_option("screened_sweep", 1)
    y3 = A3[:, 1] * 2.0 - A3[:, 2]
    ref = oracle.gomp(A3, y3, 4, 3, EPS64)
    got = d3.ctx.gomp(y3, 4, 3, EPS64)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    d.ctx.set_option("screened_sweep", 0)


def test_screened_sweep_full_size_config5_gomp(cs, oracle):
    """BASELINE configs[4] (8192 x 131072 f32, k = 512, S = 4): the screened solve equals the exact one atom for atom (insertion
    order, coefficients), certified throughout; the batch form too."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    At5, D5 = bench.make_dictionary5(cs, torch, dev)
    M5, N5, k = 8192, 131072, 512
    g = torch.Generator(device=dev).manual_seed(77)
    sel = torch.randperm(N5, generator=g, device=dev)[:k]
    sign = torch.randint(0, 2, (k,), generator=g, device=dev).to(torch.float64) * 2 - 1
    e = torch.randn(M5, generator=g, device=dev, dtype=torch.float64)
    y = ((At5[sel].to(torch.float64) * sign[:, None]).sum(0) + e * (5e-3 / e.norm())).cpu().numpy()
    exact = D5.ctx.gomp(y, 4, k, EPS32)
    for image, cert in ((2, 0), (1, 0), (3, 1)):  # (statistical int8 / bf16; RIGOROUS binary16, kept for the batch form below)
        D5.ctx.set_option("batch_cert", cert)
        D5.ctx.set_option("screened_sweep", image)
        D5.ctx.screened_stats(reset=True)
        got = D5.ctx.gomp(y, 4, k, EPS32)
        assert np.array_equal(got[2], exact[2]) and np.array_equal(got[0], exact[0]) and np.allclose(got[1], exact[1], rtol=1e-9, atol=1e-12)
        st5 = D5.ctx.screened_stats()
        assert st5["solves"] == 1 and st5["fallbacks"] <= 1, (image, st5)
    bi, bv, bn = D5.ctx.gomp_batch(np.asfortranarray(np.stack([y, -y, 0.5 * y], axis=1)), 4, k, EPS32)
    for s in range(3):
        assert bn[s] == len(exact[0]) and np.array_equal(bi[:bn[s], s], exact[0])
    assert D5.ctx.screened_stats()["fallbacks"] <= 1
    D5.close()


# ------------------------------------------------------------------ int8 screening GEMM of the batched path (CSMP_OPT_BATCH_SCREEN)
@pytest.mark.parametrize("shape", [(64, 256, 6, 5), (256, 2048, 12, 40), (130, 700, 10, 130), (512, 4096, 24, 200), (1500, 3000, 16, 9), (4096, 2500, 10, 260),
                                   (8192, 600, 6, 8), (8000, 520, 5, 3)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batched_int8_screen_matches_oracle(cs, oracle, D, shape, dtype):
    """csmp_omp_batch_mfma with int8 operands (k_b_screen256p<true>: v_mfma_i32_16x16x64_i8, exact integer accumulation, one step
    for the dictionary and one per residual): every signal's support, coefficients and count equal the oracle's; whatever the
    screen could not certify was re-solved exactly."""
    n, m, k, nsig = shape
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m, dtype=dtype)
    eps = float(np.finfo(dtype).eps)
    rng = np.random.default_rng(n * 3 + nsig)
    B = np.empty((n, nsig), order="F")
    for s in range(nsig):
        sup = rng.choice(m, size=k, replace=False)
        B[:, s] = cs.perturb(A[:, sup].astype(np.float64) @ rng.choice(np.array([-1.0, 1.0]), size=k), 5e-3, rng=rng)
    d = D(A)
    d.ctx.set_option("batch_cert", 0)  # (the int8 screen has the statistical certificate only: opt-in)
    d.ctx.set_option("batch_screen", 1)
    idx, val, nnz = d.ctx.omp_batch_mfma(B, k, eps)
    st = d.ctx.batch_stats()
    assert "i8" in d.ctx.batch_screen_kernel()
    assert st["signals"] == nsig and st["resolved_exactly"] <= st["uncertain"] + st["illcond"]
    for s in range(0, nsig, max(1, nsig // 12)):
        ref = oracle.omp(A, B[:, s], k, eps)
        assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]), s
        assert close(val[:nnz[s], s], ref[1], tight=False)
    i2, v2, n2 = d.ctx.omp_batch(B, k, eps)
    assert np.array_equal(nnz, n2) and np.array_equal(idx, i2)


@pytest.mark.parametrize("kind", ["few_valued", "partial_dct", "one_magnitude", "common_component"])
def test_batched_int8_screen_structured_dictionaries(cs, oracle, kind):
    M, N, nsig = 512, 4096, 200
    rng = np.random.default_rng(515 + len(kind))
    A = cs.structured_dictionary(kind, M, N, rng=rng)
    A64 = A.astype(np.float64)
    d = cs.Dictionary(A)
    for family, k in (("pm1", 16), ("neartie", 4)):
        B = np.empty((M, nsig), order="F")
        for s in range(nsig):
            sup = rng.choice(N, size=k, replace=False)
            x = rng.choice(np.array([-1.0, 1.0]), size=k)
            if family == "neartie":
                x = x * (1.0 + 2e-3 * rng.random(k))
            B[:, s] = cs.perturb(A64[:, sup] @ x, 5e-3, rng=rng)
        i2, v2, n2 = d.ctx.omp_batch(B, k, EPS32)
        d.ctx.set_option("batch_cert", 0)
        d.ctx.set_option("batch_screen", 1)
        idx, val, nnz = d.ctx.omp_batch_mfma(B, k, EPS32)
        st = d.ctx.batch_stats()
        print(kind, family, "int8 screen batch_stats:", st)
        assert np.array_equal(nnz, n2), (kind, family)
        assert np.array_equal(idx, i2), (kind, family, int((idx != i2).any(axis=0).sum()))
        assert np.allclose(val, v2, rtol=1e-7, atol=1e-10)
    d.close()


@pytest.mark.parametrize("shape", [(32, 64, 3), (64, 256, 8), (50, 301, 5), (256, 1024, 24), (512, 8192, 40), (640, 4096, 96), (1500, 3000, 30)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_screened_sweep_sp_matches_oracle(cs, oracle, D, shape, dtype):
    """Subspace Pursuit with the screened sweep (sp_select_screened: the top-k SET of every acquisition certified, else that
    acquisition repeated exactly): supports, coefficients and update! counts of the oracle (src/twostage.jl:42-107), both images,
    one call at a time and through csmp_sp_batch."""
    n, m, k = shape
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n * 31 + m, dtype=dtype)
    d = D(A)
    ys = []
    for seed in range(3):
        xs = cs.sparse_vector(m, k, rng=seed)
        y = A[:, xs.nzind].astype(np.float64) @ xs.nzval
        ys.append(cs.perturb(y, 5e-3 * seed, rng=seed + 50) if seed else y)
    for delta in (1e-2, 1e-12):
        refs = [oracle.sp(A, y, k, delta) for y in ys]
        for image in (3, 1, 2):
            d.ctx.set_option("screened_sweep", image)
            d.ctx.screened_stats(reset=True)
            for y, ref in zip(ys, refs):
                got = d.ctx.sp(y, k, delta)
                assert got[2] == ref[2], ("update! calls", image, delta)
                assert np.array_equal(got[0], ref[0]), (image, delta)
                assert close(got[1], ref[1], tight=False)
            st = d.ctx.screened_stats()
            assert st["solves"] >= 6, st  # (every acquisition counts: at least two per solve)
            idx, val, nnz, its = d.ctx.sp_batch(np.asfortranarray(np.stack(ys, axis=1)), k, delta)
            for s, ref in enumerate(refs):
                assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]) and its[s] == ref[2], (image, delta, s)
    d.ctx.set_option("screened_sweep", 0)


def test_screened_sweep_full_size_config5_sp(cs, oracle):
    """BASELINE configs[4] (8192 x 131072 f32, k = 512): Subspace Pursuit with the screened sweep equals the exact path (support,
    coefficients, update! calls) at both tolerances, certified (no acquisition repeated) on this dictionary."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    At5, D5 = bench.make_dictionary5(cs, torch, dev)
    M5, N5, k = 8192, 131072, 512
    g = torch.Generator(device=dev).manual_seed(78)
    sel = torch.randperm(N5, generator=g, device=dev)[:k]
    sign = torch.randint(0, 2, (k,), generator=g, device=dev).to(torch.float64) * 2 - 1
    e = torch.randn(M5, generator=g, device=dev, dtype=torch.float64)
    y = ((At5[sel].to(torch.float64) * sign[:, None]).sum(0) + e * (5e-3 / e.norm())).cpu().numpy()
    for delta in (1e-2, 1e-12):
        D5.ctx.set_option("screened_sweep", 0)
        exact = D5.ctx.sp(y, k, delta)
        for image, cert in ((2, 0), (1, 0), (3, 1)):
            D5.ctx.set_option("batch_cert", cert)
            D5.ctx.set_option("screened_sweep", image)
            D5.ctx.screened_stats(reset=True)
            got = D5.ctx.sp(y, k, delta)
            assert got[2] == exact[2] and np.array_equal(got[0], exact[0]) and np.allclose(got[1], exact[1], rtol=1e-9, atol=1e-12), (image, delta)
            st = D5.ctx.screened_stats()
            print("sp C5 screened image", image, "cert", cert, "delta", delta, st)
            assert st["solves"] == 1 + exact[2] and st["fallbacks"] <= 1, st
    bi, bv, bn, its = D5.ctx.sp_batch(np.asfortranarray(np.stack([y, -y, 0.5 * y, y], axis=1)), k, 1e-2)
    for s in range(4):
        assert bn[s] == len(exact[0]) or True
    D5.ctx.set_option("screened_sweep", 0)
    ex = D5.ctx.sp(y, k, 1e-2)
    for s in range(4):
        assert np.array_equal(bi[:bn[s], s], ex[0]), s
    D5.close()


def test_screened_sweep_mp_matches_oracle(cs, oracle, D):
    """Matching Pursuit with the screened sweep (the certified pick also selects: no guards, atoms repeat, src/matchingpursuit.jl:26-31):
    index / coefficient pairs of the oracle on both images, with a warm start, at a size where the sweep has many workgroups."""
    for (n, m, k, dtype) in [(32, 48, 30, np.float64), (64, 256, 50, np.float32), (37, 101, 25, np.float32), (512, 8192, 40, np.float32)]:
        A, x, b = cs.sparse_data(n=n, m=m, k=3, rng=n + m, dtype=dtype)
        b = cs.perturb(b, 5e-2, rng=1)
        d = D(A)
        ref = oracle.mp(A, b, k)
        for image in (3, 1, 2):
            d.ctx.set_option("screened_sweep", image)
            d.ctx.screened_stats(reset=True)
            got = d.ctx.mp(b, k)
            assert np.array_equal(got[0], ref[0]), (n, m, image)
            assert close(got[1], ref[1])
            x1 = cs.mp(d, b, 7)
            x2 = cs.mp(d, b, k - 7, x1)
            assert np.array_equal(x2.nzind, ref[0]) and close(x2.nzval, ref[1])
            assert d.ctx.screened_stats()["solves"] == 3
        d.ctx.set_option("screened_sweep", 0)


def test_batched_screen_auto_rule(cs, oracle, D):
    """CSMP_OPT_BATCH_SCREEN = 2 under the statistical certificate (both opt-in): int8 operands where the dictionary is flat, bf16 where a few large entries would
    coarsen the common int8 step (spikes beside a dense basis).  Forced int8 on such a dictionary still returns the exact path's
    results -- through the certificate and the exact re-solves."""
    rng = np.random.default_rng(31)
    M, k, nsig = 256, 8, 40
    G = rng.standard_normal((M, 768))
    G /= np.linalg.norm(G, axis=0)
    A_flat = np.asfortranarray(G.astype(np.float32))
    A_spiky = np.asfortranarray(np.hstack([np.eye(M), G]).astype(np.float32))  # [I, G]: max|A| / rms = sqrt(M)
    for A, expect_i8 in ((A_flat, True), (A_spiky, False)):
        d = D(A)
        d.ctx.set_option("batch_cert", 0)
        d.ctx.set_option("batch_screen", 2)
        B = np.empty((M, nsig), order="F")
        for s in range(nsig):
            sup = rng.choice(A.shape[1], size=k, replace=False)
            B[:, s] = cs.perturb(A[:, sup].astype(np.float64) @ rng.choice(np.array([-1.0, 1.0]), size=k), 5e-3, rng=rng)
        i2, v2, n2 = d.ctx.omp_batch(B, k, EPS32)
        idx, val, nnz = d.ctx.omp_batch_mfma(B, k, EPS32)
        assert ("i8" in d.ctx.batch_screen_kernel()) == expect_i8, d.ctx.batch_screen_kernel()
        assert np.array_equal(nnz, n2) and np.array_equal(idx, i2) and np.allclose(val, v2, rtol=1e-7, atol=1e-10)
        for s in range(0, nsig, 10):
            ref = oracle.omp(A, B[:, s], k, EPS32)
            assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0])
        d.ctx.set_option("batch_screen", 1)  # forced int8, whatever the dictionary looks like
        idx, val, nnz = d.ctx.omp_batch_mfma(B, k, EPS32)
        st = d.ctx.batch_stats()
        assert "i8" in d.ctx.batch_screen_kernel()
        assert np.array_equal(nnz, n2) and np.array_equal(idx, i2) and np.allclose(val, v2, rtol=1e-7, atol=1e-10), st
        d.ctx.set_option("batch_screen", 1)
        d.ctx.set_option("batch_cert", 1)  # under the rigorous certificate an int8 request runs the default operands
        idx, val, nnz = d.ctx.omp_batch_mfma(B, k, EPS32)
        assert "i8" not in d.ctx.batch_screen_kernel()
        assert np.array_equal(nnz, n2) and np.array_equal(idx, i2) and np.allclose(val, v2, rtol=1e-7, atol=1e-10)
        d.ctx.set_option("batch_screen", DEFAULT_SCREEN)


def test_screened_sweep_int8_image_only_on_flat_dictionaries(cs, oracle, D):
    """CSMP_OPT_SCREENED_SWEEP = 2 on a dictionary with spikes beside a dense basis ([I, G]: max|A| / rms = sqrt(M)): one int8 step
    would leave the dense atoms a handful of levels, so the sweeps read the bf16 image instead -- the picks certify (no solve is
    repeated) and the results are the oracle's."""
    rng = np.random.default_rng(32)
    M, k = 256, 8
    G = rng.standard_normal((M, 768))
    G /= np.linalg.norm(G, axis=0)
    A = np.asfortranarray(np.hstack([np.eye(M), G]).astype(np.float32))
    d = D(A)
    d.ctx.set_option("batch_cert", 0)  # (the statistical certificate: the claim "the picks certify" is about it)
    d.ctx.set_option("screened_sweep", 2)
    d.ctx.screened_stats(reset=True)
    for s in range(6):
        sup = rng.choice(A.shape[1], size=k, replace=False)
        y = cs.perturb(A[:, sup].astype(np.float64) @ rng.choice(np.array([-1.0, 1.0]), size=k), 5e-3, rng=rng)
        ref = oracle.omp(A, y, k, EPS32)
        got = d.ctx.omp(y, k, EPS32)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and close(got[1], ref[1], tight=False)
    st = d.ctx.screened_stats()
    assert st["solves"] == 6 and st["fallbacks"] <= 1, st
    d.ctx.set_option("screened_sweep", 0)


@pytest.mark.parametrize("cfg", [(32, 64, 3, np.float64), (128, 512, 12, np.float32), (100, 333, 9, np.float64), (256, 2048, 40, np.float32), (512, 8192, 48, np.float32)])
def test_screened_sweep_ompr_matches_oracle(cs, oracle, D, cfg):
    """OMP with replacement on the screened sweep (certified top-k of the oblivious acquisition, certified arg-max of every update!,
    exact correlations on the support; an uncertified sweep repeated exactly on the spot): supports, coefficients and iteration
    counts of the oracle (src/twostage.jl:110-202) on both images, noisy signals that make the replacement loop work."""
    n, m, k, dtype = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + m + k, dtype=dtype)
    d = D(A)
    for seed, noise in ((0, 0.0), (1, 5e-3), (2, 2e-1)):
        xs = cs.sparse_vector(m, k + 2, rng=seed)
        y = A[:, xs.nzind].astype(np.float64) @ xs.nzval
        if noise:
            y = cs.perturb(y, noise, rng=seed + 50)
        ref = oracle.ompr(A, y, k, 1e-6, -1)
        for image in (3, 1, 2):
            d.ctx.set_option("screened_sweep", image)
            got = d.ctx.ompr(y, k, 1e-6)
            assert np.array_equal(got[0], ref[0]), (seed, image, got, ref)
            assert close(got[1], ref[1], tight=False)
            assert got[2] == ref[2], "iterations"
        d.ctx.set_option("screened_sweep", 0)


# ---- adversarial residuals for the screening certificates (round 4) -------------------------------------------------------------
def _bf16_image(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32).astype(np.float64)


def _f16_image(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def _round_to_worst_case(b0, want, bits):
    """Every entry of b0 moved (by less than one unit in its `bits`-bit significand) to just beside a rounding MIDPOINT of the
    `bits`-bit format, on the side that makes its rounding error f = b - image(b) carry the sign `want`: |f_i| = half an ulp,
    all signs chosen by the adversary -- the worst case of a round-to-nearest image of the residual."""
    mag = np.abs(b0)
    ex = np.floor(np.log2(np.maximum(mag, 1e-300)))
    ulp = 2.0 ** (ex - (bits - 1))
    lo = np.floor(mag / ulp) * ulp  # grid point at or below |b|
    mid = lo + ulp / 2
    tiny = ulp / 64
    sgn = np.where(b0 < 0, -1.0, 1.0)
    # |b| just below the midpoint -> rounds toward zero -> f = +sgn (ulp/2 - tiny); just above -> f = -sgn (ulp/2 - tiny)
    out = sgn * np.where(sgn * want > 0, mid - tiny, mid + tiny)
    return np.where(want == 0, b0, out)


def _adversarial_signal(A, i1, i2, image, bits, alpha=0.1, mu=1.0):
    """b with exact |<a2, b>| > |<a1, b>| by a hair, both far above every other atom, whose IMAGE products invert the order by as
    much as a round-to-nearest image allows: b = alpha1 a1 + alpha2 a2 + mu (e2 - e1)/|e2 - e1| with e_i = a_i - image(a_i) (the
    dictionary side: <image(a_i), b> = <a_i, b> - <e_i, b>), every entry then placed beside a rounding midpoint so that the
    residual's own rounding error has the sign of a2 - a1 (the residual side).  VERDICT round 3, "Next round" item 3."""
    a1, a2 = A[:, i1].astype(np.float64), A[:, i2].astype(np.float64)
    e1, e2 = a1 - image(A[:, i1]), a2 - image(A[:, i2])
    eh = e2 - e1
    eh /= max(np.linalg.norm(eh), 1e-300)
    al1 = al2 = alpha
    rho = float(a1 @ a2)
    for _ in range(40):
        b = _round_to_worst_case(al1 * a1 + al2 * a2 + mu * eh, np.sign(a2 - a1), bits)
        g = (abs(float(a2 @ b)) - abs(float(a1 @ b))) / np.linalg.norm(b)  # want: 0 < g < 2e-4
        if 2e-5 < g < 2e-4:
            ex = np.abs(A.astype(np.float64).T @ b)
            third = np.partition(ex, -3)[-3]
            return b if third < 0.8 * ex[i1] else None  # (None: a third atom came close by chance -- the caller takes another pair)
        al2 += (1e-4 - g) * np.linalg.norm(b) / (1.0 - abs(rho))
    raise AssertionError("adversarial construction did not converge")


@pytest.mark.parametrize("image_name", ["bf16", "f16"])
def test_batched_certificate_against_adversarial_residuals(cs, oracle, image_name):
    """The batched path's DEFAULT certificate must not be breakable: signals constructed so that the screen's rounding errors are
    coherent and worst-case (see _adversarial_signal) -- the exact arg-max (src/matchingpursuit.jl:181-185) hides behind a
    near-tied atom whose screened value is pushed up while its own is pushed down.  Under the library's defaults every first
    pick and every k = 6 support must be the oracle's.  The same batch is then run under the opt-in statistical certificates
    (bf16 and int8 operands) and the outcome is REPORTED (not asserted): a wrong support with `uncertain == 0` there is the
    reason those modes are opt-in."""
    M, N, nadv, k = 4096, 2048, 24, 6
    rng = np.random.default_rng(2024)
    A = rng.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0)
    A = np.asfortranarray(A.astype(np.float32))
    image, bits = (_bf16_image, 8) if image_name == "bf16" else (_f16_image, 11)
    cols, sig = [], []
    for i1, i2 in rng.permutation(N)[:8 * nadv].reshape(-1, 2):
        b = _adversarial_signal(A, int(i1), int(i2), image, bits)
        if b is not None and len(sig) < nadv:
            cols.append((int(i1), int(i2)))
            sig.append(b)
    assert len(sig) == nadv
    # the construction does what it says (checked here in numpy, so a pass below means something): exact order a2 > a1,
    # image order a1 > a2 by more than the image's typical rounding noise
    A64 = A.astype(np.float64)
    Aimg = np.stack([image(A[:, j]) for j in range(N)], axis=1)
    inverted = 0
    for (i1, i2), b in zip(cols, sig):
        ex, sc = np.abs(A64.T @ b), np.abs(Aimg.T @ image(b))
        assert int(np.argmax(ex)) == i2 and ex[i2] > ex[i1]
        inverted += int(np.argmax(sc) == i1)
    assert inverted == nadv, inverted
    # the adversarial signals sit among ordinary planted ones
    B = [cs.perturb(A64 @ cs.sparse_vector(N, k, rng=rng).to_dense(), 5e-3, rng=rng) for _ in range(40)]
    where = sorted(rng.permutation(len(B) + nadv)[:nadv].tolist())
    for w, b in zip(where, sig):
        B.insert(w, b)
    B = np.asfortranarray(np.stack(B, axis=1))
    refs = [oracle.omp(A, B[:, s], k, EPS32) for s in range(B.shape[1])]
    d = cs.Dictionary(A)

    def run(kk):
        idx, val, nnz = d.ctx.omp_batch_mfma(B, kk, EPS32)
        st = d.ctx.batch_stats()
        wrong = [s for s in range(B.shape[1]) if not (nnz[s] == min(kk, len(refs[s][0])) and (
            np.array_equal(idx[:nnz[s], s], refs[s][0]) if kk == k else int(idx[0, s]) == int(refs[s][2][0])))]
        return wrong, st, val, nnz

    # (1) the library's defaults, and the rigorous certificate with each 16-bit operand type: never wrong
    for name, cert, screen in (("defaults", None, None), ("rigorous bf16", 1, 0), ("rigorous binary16", 1, 3)):
        if cert is not None:
            d.ctx.set_option("batch_cert", cert)
            d.ctx.set_option("batch_screen", screen)
        for kk in (1, k):
            wrong, st, val, nnz = run(kk)
            print("adversarial[%s] %s, k=%d: %s wrong %s" % (image_name, name, kk, d.ctx.batch_screen_kernel().split(" ")[0], wrong), st)
            assert wrong == [], (name, kk, wrong, st)
        for s in range(B.shape[1]):
            assert close(val[:nnz[s], s], refs[s][1], tight=False), s
    # (2) the opt-in statistical certificates, reported
    for name, cert, screen in (("statistical bf16", 0, 0), ("statistical binary16", 0, 3), ("statistical int8", 0, 1)):
        d.ctx.set_option("batch_cert", cert)
        d.ctx.set_option("batch_screen", screen)
        wrong, st, _, _ = run(1)
        print("adversarial[%s] opt-in %s: first pick wrong on %d of %d adversarial signals, uncertain %d -> %s" % (
            image_name, name, len(wrong), nadv, st["uncertain"],
            "SILENTLY WRONG (why this mode is opt-in)" if wrong else "held on this construction"))
        assert set(wrong) <= set(where)  # ordinary signals are never affected
    d.close()


@pytest.mark.parametrize("image_name", ["bf16", "f16"])
def test_screened_sweep_certificate_against_adversarial_residuals(cs, oracle, image_name):
    """The same construction against the opt-in screened SINGLE-SIGNAL sweep (CSMP_OPT_SCREENED_SWEEP: the sweep reads an image of
    A, the pick is certified, an uncertified solve is repeated exactly).  Under the rigorous certificate every first pick and every
    k = 6 support must be the oracle's, whatever the image; the statistical certificate is run on the same signals and its
    outcome reported."""
    M, N, nadv, k = 4096, 2048, 12, 6
    rng = np.random.default_rng(4048)
    A = rng.standard_normal((M, N))
    A /= np.linalg.norm(A, axis=0)
    A = np.asfortranarray(A.astype(np.float32))
    image, bits, opt = (_bf16_image, 8, 1) if image_name == "bf16" else (_f16_image, 11, 3)
    sig = []
    for i1, i2 in rng.permutation(N)[:8 * nadv].reshape(-1, 2):
        b = _adversarial_signal(A, int(i1), int(i2), image, bits)
        if b is not None and len(sig) < nadv:
            sig.append(b)
    assert len(sig) == nadv
    refs = [oracle.omp(A, b, k, EPS32) for b in sig]
    d = cs.Dictionary(A)
    d.ctx.set_option("screened_sweep", opt)
    for cert in (1, 0):
        d.ctx.set_option("batch_cert", cert)
        d.ctx.screened_stats(reset=True)
        wrong = []
        for s, b in enumerate(sig):
            for kk in (1, k):
                g = d.ctx.omp(b, kk, EPS32)
                ok = int(g[2][0]) == int(refs[s][2][0]) if kk == 1 else (np.array_equal(g[0], refs[s][0]) and close(g[1], refs[s][1], tight=False))
                if not ok:
                    wrong.append((s, kk))
        st = d.ctx.screened_stats()
        print("adversarial screened sweep [%s] %s certificate: wrong %s, %s" % (image_name, "rigorous" if cert else "statistical (opt-in)", wrong, st))
        if cert == 1:
            assert wrong == [], (wrong, st)
    d.close()


def test_omp_sharded_in_library_rccl(cs, oracle, D):
    """csmp_comm_id / csmp_comm_init / csmp_omp_sharded: the signal-sharded solve with the ONE collective (ncclAllGather) inside the
    library.  One GPU can only hold a group of one rank (RCCL refuses two ranks on a device), which still runs every line: the
    lazy binding of librccl, the communicator, the device-side packing, the collective on the context's stream, the unpacking
    into global order.  Results: csmp_omp_batch's and the oracle's."""
    import torch
    A, x, b = cs.sparse_data(n=256, m=2048, k=8, rng=42, dtype=np.float32)
    M, k, nsig = 256, 8, 11
    rng = np.random.default_rng(5)
    B = np.asfortranarray(np.stack([cs.perturb(A.astype(np.float64) @ cs.sparse_vector(2048, k, rng=rng).to_dense(), 5e-3, rng=rng)
                                    for _ in range(nsig)], axis=1))
    d = D(A)
    with pytest.raises(cs.CsmpError):  # no communicator yet
        d.ctx.omp_sharded(B, nsig, k, EPS32)
    cid = cs.comm_id()
    assert len(cid) == 128 and any(cid)
    d.ctx.comm_init(cid, 0, 1)
    i2, v2, n2 = d.ctx.omp_batch(B, k, EPS32)
    for method in ("exact", "mfma"):
        idx, val, nnz = d.ctx.omp_sharded(B, nsig, k, EPS32, method)
        assert np.array_equal(nnz, n2) and np.array_equal(idx, i2) and np.allclose(val, v2, rtol=1e-9, atol=1e-12), method
        Bd = torch.from_numpy(np.ascontiguousarray(B.T)).cuda()
        di = torch.full((nsig, k), -7, dtype=torch.int64, device="cuda")
        dv = torch.zeros((nsig, k), dtype=torch.float64, device="cuda")
        dn = torch.zeros(nsig, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        d.ctx.omp_sharded_device(Bd, nsig, k, EPS32, di, dv, dn, method)
        assert np.array_equal(di.cpu().numpy().T, i2) and np.array_equal(dn.cpu().numpy(), n2)
    for s in range(nsig):
        ref = oracle.omp(A, B[:, s], k, EPS32)
        assert nnz[s] == len(ref[0]) and np.array_equal(idx[:nnz[s], s], ref[0]) and close(val[:nnz[s], s], ref[1], tight=False)
    d.ctx.comm_free()
    with pytest.raises(cs.CsmpError):
        d.ctx.omp_sharded(B, nsig, k, EPS32)
    d.ctx.comm_init(cs.comm_id(), 0, 1)  # a second communicator on the same context; freed by csmp_destroy
    # a rank whose LOCAL solve fails must not leave before the collective (the others would wait in the
    # all-gather for ever): it sends a block that carries its status, and every rank returns that status after the gather.  Injected
    # here with a leading dimension below M (csmp_omp_batch: CSMP_EDIM) -- the call comes back, with the local code and message, and
    # the communicator is as usable as before.
    import ctypes as C
    from csmp_pkg import load
    L = load()._lib
    idx = np.zeros((k, nsig), np.int64, order="F")
    val = np.zeros((k, nsig), np.float64, order="F")
    nnz = np.zeros(nsig, np.int64)
    with pytest.raises(cs.CsmpError) as e:
        d.ctx.call("csmp_omp_sharded", L.ptr(B), L.F64, L.i64(M - 1), L.i64(nsig), L.HOST, L.i64(k), C.c_double(EPS32), 0, L.ptr(idx), L.ptr(val), L.ptr(nnz), L.HOST)
    assert e.value.code in (L.EDIM, L.EINVAL)  # (csmp_omp_batch reports a short leading dimension as a bad argument)
    with pytest.raises(cs.CsmpError) as e:  # ... and with a missing block
        d.ctx.call("csmp_omp_sharded", None, L.F64, L.i64(M), L.i64(nsig), L.HOST, L.i64(k), C.c_double(EPS32), 0, L.ptr(idx), L.ptr(val), L.ptr(nnz), L.HOST)
    assert e.value.code == L.EINVAL and "B == NULL" in str(e.value)
    idx, val, nnz = d.ctx.omp_sharded(B, nsig, k, EPS32)
    assert np.array_equal(nnz, n2) and np.array_equal(idx, i2)
    # Round 6 (verdict item 8, advisor): arguments are no longer checked in front of the collectives -- a rank with a bad k or eps
    # would leave while ranks with good ones wait.  They travel in the fixed-size agreement exchange; the verdict comes back from it.
    for bad_k, bad_eps, bad_dtype in ((0, EPS32, L.F64), (k, -1.0, L.F64), (k, EPS32, 7)):
        with pytest.raises(cs.CsmpError) as e:
            d.ctx.call("csmp_omp_sharded", L.ptr(B), bad_dtype, L.i64(M), L.i64(nsig), L.HOST, L.i64(bad_k), C.c_double(bad_eps), 0, L.ptr(idx), L.ptr(val),
                       L.ptr(nnz), L.HOST)
        assert e.value.code == L.EINVAL
    d.ctx.call("csmp_omp_sharded", L.ptr(B), L.F64, L.i64(M), L.i64(0), L.HOST, L.i64(k), C.c_double(EPS32), 0, L.ptr(idx), L.ptr(val), L.ptr(nnz), L.HOST)  # an empty batch
    # A REAL allocation failure inside the block's solves (csmp_tune fail_alloc: hipMalloc of an impossible size -- hipErrorOutOfMemory
    # stays pending, as on a full device): the rank must still reach the gather and return ITS failure (a HIP error read back in front
    # of the gather would have made it leave, with CSMP_EHIP), and the context and communicator work afterwards.
    for method in ("exact", "mfma"):
        e2 = cs.Dictionary(A)
        e2.ctx.comm_init(cs.comm_id(), 0, 1)
        e2.ctx.tune("fail_alloc", 3)
        with pytest.raises(cs.CsmpError) as e:
            e2.ctx.omp_sharded(B, nsig, k, EPS32, method)
        assert e.value.code == L.EHIP and "hipMalloc" in str(e.value), (e.value.code, str(e.value))
        e2.ctx.tune("fail_alloc", 0)
        idx, val, nnz = e2.ctx.omp_sharded(B, nsig, k, EPS32, method)
        assert np.array_equal(nnz, n2) and np.array_equal(idx, i2), method
        e2.close()


@pytest.mark.parametrize("cfg", [(2304, 4608, 1100, 2, 4), (4096, 8192, 2048, 1, 2)])
def test_srr_and_ompr_beyond_1023_columns(cs, oracle, cfg):
    """The two-stage solvers' supports are bounded by size(A,1) in the reference (src/twostage.jl:3-33,110-202); rounds 1-3 capped
    them at 1023 columns (one thread per column in the removal kernels).  The explicit-inverse removal now scans four columns per
    thread (k_tdel_prep<4>) and builds T = R^-1 with up to 64 entries per lane (k_tinv_build_big): srr at k = 2048, M = 4096 --
    oblivious start, forward + backward steps, supports, coefficients and iteration counts against the oracle (a bounded number of
    iterations: the oracle refactorises from scratch at every change)."""
    n, m, k, l, maxiter = cfg
    A, x, b = cs.sparse_data(n=n, m=m, k=k, rng=n + k, dtype=np.float32)
    xs = cs.sparse_vector(m, k + 2, rng=1)
    y = cs.perturb(A[:, xs.nzind].astype(np.float64) @ xs.nzval, 5e-3, rng=2)
    d = cs.Dictionary(A)
    ref = oracle.srr(A, y, k, 1e-12, maxiter, 1, l)
    got = d.ctx.srr(y, k, 1e-12, maxiter, 1, l)
    assert len(got[0]) == k and np.array_equal(got[0], ref[0]), int((got[0] != ref[0]).sum())
    assert close(got[1], ref[1], tight=False) and got[2] == ref[2]
    if k <= 1100:  # ompr on the same data: the exchange steps go through the same removal kernels
        ro = oracle.ompr(A, y, k, 1e-6, 3)
        go = d.ctx.ompr(y, k, 1e-6, 3)
        assert np.array_equal(go[0], ro[0]) and close(go[1], ro[1], tight=False) and go[2] == ro[2]
    d.close()


@pytest.mark.parametrize("cfg", [(11, 3, 5), (8, 8, 4), (5, 8, 3), (64, 4, 16), (1, 1, 2), (7, 2, 1)])
def test_sharded_wire_layout_on_the_device_for_several_ranks(cs, D, cfg):
    """The device-side halves of csmp_omp_sharded (k_pack_rows / k_unpack_rows) for world > 1 -- which RCCL cannot exercise on one GPU:
    every "rank" packs its contiguous block (csmp_shard_range) padded to ceil(nsig / world) rows, the blocks are concatenated as
    an all-gather would deliver them, and the unpacked arrays must be the original ones in global signal order; the rows equal the
    host packer's (csmp_pack_results), so both paths speak one wire layout."""
    import torch
    nsig, world, k = cfg
    A, x, b = cs.sparse_data(n=32, m=64, k=2, rng=1, dtype=np.float32)
    d = D(A)
    rng = np.random.default_rng(nsig * 31 + world)
    nnz = rng.integers(0, k + 1, size=nsig)
    idx = np.full((nsig, k), -1, np.int64)
    val = np.zeros((nsig, k))
    for s in range(nsig):
        idx[s, :nnz[s]] = np.sort(rng.choice(10_000_000, size=nnz[s], replace=False))
        val[s, :nnz[s]] = rng.standard_normal(nnz[s])
    rows = -(-nsig // world)
    blocks = []
    for r in range(world):
        lo, hi = cs.shard_range(nsig, r, world)
        ti, tv, tn = (torch.from_numpy(np.ascontiguousarray(a[lo:hi])).cuda() for a in (idx, val, nnz.astype(np.int64)))
        pk = d.ctx.pack_block_device(ti, tv, tn, rows)
        d.ctx.sync()
        host = cs.sharded.pack(idx[lo:hi].T, val[lo:hi].T, nnz[lo:hi]) if hi > lo else np.zeros((0, 2 * k + 1))
        assert np.array_equal(pk.cpu().numpy()[:hi - lo], host) and not pk.cpu().numpy()[hi - lo:].any()
        blocks.append(pk)
    gi, gv, gn = d.ctx.unpack_gathered_device(torch.cat(blocks, dim=0).contiguous(), k, nsig, world)
    d.ctx.sync()
    assert np.array_equal(gn.cpu().numpy(), nnz)
    for s in range(nsig):
        assert np.array_equal(gi[s, :nnz[s]].cpu().numpy(), idx[s, :nnz[s]]) and np.array_equal(gv[s, :nnz[s]].cpu().numpy(), val[s, :nnz[s]])
