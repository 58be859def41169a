"""csmp_sbl at the benchmark's shape (4096 x 65536 Float32) and at 1024 x 16384.

    python tools/bench_sbl.py --mode update [--small]   # seconds of one update (csmp_sbl, maxiter = 1); its stages by HIP events (the weighted
                                                        # Gram matrix, the factorisation, k_sbl_forms: csmp_bench_sbl); k_ard_forms per block of
                                                        # 128 directions in the same run (csmp_bench_ard_forms), and k_sbl_forms against it
    python tools/bench_sbl.py --mode torch [--small]    # the same Woodbury update as a PyTorch user writes it, Float64 on the card
                                                        # (torch.linalg.cholesky, solve_triangular), and the library's x and γ against it
    python tools/bench_sbl.py --mode solve [--small]    # sbl on a planted signal: updates, seconds, the support found
    python tools/bench_sbl.py --mode all [--out profiles/r17_sbl.json]

all runs every step in a fresh child process under a time limit of its own and stops at the first that fails.  No thresholds.  Needs a
GPU; there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"large": (4096, 65536), "small": (1024, 16384)}
SIGMA = 1e-2
ARD_K = 1024  # directions of the k_ard_forms run it is compared with (profiles/r14_reweight.json's larger support)


def make_inputs(M, N, k=64):
    """unit-norm Gaussian atoms generated on the device ((N, M): rows are atoms), a planted ±1 signal on k atoms, y = A x + noise of norm σ / 2"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(17)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float32)
    At /= At.norm(dim=1, keepdim=True)
    At = At.contiguous()
    S = torch.sort(torch.randperm(N, generator=g, device="cuda")[:k]).values
    x0 = torch.zeros(N, dtype=torch.float64, device="cuda")
    x0[S] = torch.where(torch.rand(k, generator=g, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
    e = torch.randn(M, generator=g, device="cuda", dtype=torch.float64)
    y = x0[S] @ At[S].to(torch.float64) + e * (SIGMA / 2 / float(e.norm()))
    return At, S, y


def load():
    sys.path.insert(0, HERE)
    from csmp_pkg import load as ld
    return ld()


def med(v):
    return sorted(v)[len(v) // 2]


def dense_row_blocks(M):
    nrb, nblk = (M + 63) // 64, (M + 127) // 128
    return nblk * nrb, sum(min(nrb, 2 * (d + 1)) for d in range(nblk))


def mode_update(M, N, calls):
    import torch
    cs = load()
    At, S, y = make_inputs(M, N)
    d = cs.Dictionary(At)
    x = torch.empty(N, dtype=torch.float64, device="cuda")
    gam = torch.ones(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res = {"mode": "update", "shape": [M, N, "float32"], "device": d.ctx.device_info()[0]}
    d.ctx.sbl_device(y, SIGMA ** 2, x, None, gam, maxiter=1, min_change=0.0)  # warm-up: buffers, code objects; γ after one update
    secs = []
    for _ in range(calls):
        t0 = time.perf_counter()
        d.ctx.sbl_device(y, SIGMA ** 2, x, gam, None, maxiter=1, min_change=0.0)  # (returns with the work done)
        secs.append(time.perf_counter() - t0)
    res["update_seconds"] = secs
    res["update_seconds_median"] = med(secs)
    res["stages_ms"] = d.ctx.bench_sbl(SIGMA ** 2, max(calls, 3))
    dense, run = dense_row_blocks(M)
    res["forms_row_blocks_dense"], res["forms_row_blocks_run"] = dense, run
    forms_ms = res["stages_ms"]["forms_ms"]
    res["forms_ms_per_128_directions"] = forms_ms / ((M + 127) // 128)
    res["forms_flop_per_s_of_the_blocks_run"] = 2.0 * 128 * 64 * run * N / (forms_ms * 1e-3)
    res["gram_flop_per_s_of_the_upper_tiles"] = 2.0 * 128 * 128 * (((M + 127) // 128) * ((M + 127) // 128 + 1) // 2) * N / (res["stages_ms"]["gram_ms"] * 1e-3)
    # k_ard_forms in the same run: a dense pass over min(M, 1024) directions
    k = min(M, ARD_K)
    xs = torch.zeros(N, dtype=torch.float64, device="cuda")
    xs[torch.randperm(N, device="cuda")[:k]] = 1.0
    w = torch.ones(N, dtype=torch.float64, device="cuda")
    d.ctx.ard_weights_device(xs, w, torch.empty_like(w), 1e-2, 1)
    ard_ms, _ = d.ctx.bench_ard_forms(0, max(calls, 3), 1e-2)
    per_block = ard_ms / ((k + 127) // 128)
    res["k_ard_forms_k"] = k
    res["k_ard_forms_ms"] = ard_ms
    res["k_ard_forms_ms_per_128_directions"] = per_block
    res["dense_pass_ms_arithmetic"] = per_block * ((M + 127) // 128)  # arithmetic: k_ard_forms's time per block times ceil(M / 128) blocks
    res["forms_over_dense_pass"] = forms_ms / res["dense_pass_ms_arithmetic"]
    d.close()
    return res


def woodbury(At64, y, gam, s2):
    """C = σ² I + A Γ Aᵀ (M x M), Cholesky, the projections of every atom in blocks of 8192: (x, γ⁺)"""
    import torch
    N, M = At64.shape
    C = s2 * torch.eye(M, dtype=torch.float64, device="cuda") + At64.T @ (At64 * gam[:, None])
    L = torch.linalg.cholesky(C)
    t = torch.linalg.solve_triangular(L, y[:, None], upper=False)[:, 0]
    s = torch.empty(N, dtype=torch.float64, device="cuda")
    q = torch.empty(N, dtype=torch.float64, device="cuda")
    for j0 in range(0, N, 8192):
        P = torch.linalg.solve_triangular(L, At64[j0:j0 + 8192].T, upper=False)
        s[j0:j0 + 8192] = (P * P).sum(dim=0)
        q[j0:j0 + 8192] = t @ P
    return gam * q, gam * q * q / s + 1e-14


def mode_torch(M, N, calls):
    import torch
    cs = load()
    At, S, y = make_inputs(M, N)
    d = cs.Dictionary(At)
    At64 = At.to(torch.float64)
    res = {"mode": "torch", "shape": [M, N, "float32"]}
    x = torch.empty(N, dtype=torch.float64, device="cuda")
    g1 = torch.empty(N, dtype=torch.float64, device="cuda")
    g2 = torch.empty(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d.ctx.sbl_device(y, SIGMA ** 2, x, None, g1, maxiter=1, min_change=0.0)  # γ after one update: a spread of variances
    d.ctx.sbl_device(y, SIGMA ** 2, x, g1, g2, maxiter=1, min_change=0.0)
    secs = []
    for _ in range(calls + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xt, gt = woodbury(At64, y, g1, SIGMA ** 2)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    res["torch_woodbury_update_seconds_median"] = med(secs[1:])
    res["library_against_torch_max_abs_diff_of_x"] = float((x - xt).abs().max())
    res["max_abs_x"] = float(xt.abs().max())
    res["library_against_torch_max_abs_diff_of_gamma"] = float((g2 - gt).abs().max())
    res["max_gamma"] = float(gt.max())
    d.close()
    return res


def mode_solve(M, N, maxiter):
    import torch
    cs = load()
    At, S, y = make_inputs(M, N)
    d = cs.Dictionary(At)
    x = torch.empty(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d.ctx.sbl_device(y, SIGMA ** 2, x, maxiter=1)  # warm-up
    t0 = time.perf_counter()
    info = d.ctx.sbl_device(y, SIGMA ** 2, x, maxiter=maxiter)
    secs = time.perf_counter() - t0
    found = torch.nonzero(x.abs() > SIGMA).flatten()
    res = {"mode": "solve", "shape": [M, N, "float32"], "planted": int(S.numel()), "maxiter": maxiter, "updates": info["iterations"],
           "converged": info["converged"], "solve_seconds": secs, "seconds_per_update": secs / max(info["iterations"], 1),
           "support_is_planted": bool(torch.equal(found, S)), "entries_above_sigma": int(found.numel())}
    d.close()
    return res


def child(args, limit):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("update", "torch", "solve", "all"), default="update")
    ap.add_argument("--small", action="store_true", help="1024 x 16384 instead of 4096 x 65536")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=24, help="most updates of --mode solve")
    ap.add_argument("--out")
    a = ap.parse_args()
    M, N = SHAPES["small" if a.small else "large"]
    if a.mode == "update":
        print(json.dumps(mode_update(M, N, a.calls)))
    elif a.mode == "torch":
        print(json.dumps(mode_torch(M, N, a.calls)))
    elif a.mode == "solve":
        print(json.dumps(mode_solve(M, N, a.maxiter)))
    else:
        res = {"sigma": SIGMA}

        def save():
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)

        for size, flag, limit in (("small", ["--small"], 180), ("large", [], 300)):
            for mode in ("update", "torch", "solve"):
                res[f"{mode}_{size}"] = child(["--mode", mode, "--calls", str(a.calls), "--maxiter", str(a.maxiter)] + flag, limit)
                if mode == "update":
                    res["measured_on"] = res[f"{mode}_{size}"]["device"]
                save()
                print(f"{mode}_{size}", json.dumps({u: v for u, v in res[f"{mode}_{size}"].items() if not isinstance(v, list)}), flush=True)


if __name__ == "__main__":
    main()
