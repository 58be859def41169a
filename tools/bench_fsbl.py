"""csmp_fsbl / csmp_rmps at the benchmark's shape (4096 x 65536 Float32) and at 2048 x 32768 Float64.

    python tools/bench_fsbl.py --mode step [--f64]    # seconds of one greedy step (the difference of two csmp_fsbl runs with different
                                                      # maxiter, per pass); its parts by HIP events (csmp_bench_fsbl: the N-pass and pick,
                                                      # the column and v = C^-1 a_i, the rank-one update of C^-1, the sweep w = A'v) and
                                                      # each part's bytes of the traffic model over its time, as a fraction of 8 TB/s
    python tools/bench_fsbl.py --mode torch [--f64]   # the same step as a PyTorch user writes it, Float64 on the card, and the library's
                                                      # history and x against a run of that restatement
    python tools/bench_fsbl.py --mode solve [--f64]   # fsbl and rmps on a planted signal: steps, seconds, the support found
    python tools/bench_fsbl.py --mode all [--out profiles/r18_fsbl.json]

all runs every step in a fresh child process under a time limit of its own and stops at the first that fails.  No thresholds.  Needs a
GPU; there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"f32": (4096, 65536, "float32"), "f64": (2048, 32768, "float64")}
SIGMA = 1e-2
HBM_PEAK = 8e12   # bytes / s, the nominal peak the other sections of DESIGN.md measure against
K = 64            # planted atoms
T0, T1 = 8, 40    # passes of the two timed runs: every pass in between adds an atom


def make_inputs(M, N, dtype, k=K):
    """unit-norm Gaussian atoms generated on the device ((N, M): rows are atoms), a planted ±1 signal on k atoms, y = A x + noise of norm σ / 2"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(17)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float32)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(getattr(torch, dtype)).contiguous()
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


def mode_step(M, N, dtype, calls):
    import torch
    cs = load()
    At, S, y = make_inputs(M, N, dtype)
    d = cs.Dictionary(At)
    x = torch.empty(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res = {"mode": "step", "shape": [M, N, dtype], "device": d.ctx.device_info()[0]}
    d.ctx.fsbl_device(y, SIGMA ** 2, x, maxiter=2)  # warm-up: buffers, code objects

    def run(t):
        t0 = time.perf_counter()
        info = d.ctx.fsbl_device(y, SIGMA ** 2, x, maxiter=t, history_cap=t)  # (returns with the work done)
        return time.perf_counter() - t0, info

    short, long_ = [], []
    for _ in range(calls):
        s, i0 = run(T0)
        l, i1 = run(T1)
        short.append(s)
        long_.append(l)
    assert len(i0["history"]) == T0 and len(i1["history"]) == T1  # every pass applied a step
    res["passes"] = [T0, T1]
    res["run_seconds"] = [short, long_]
    res["step_seconds"] = (med(long_) - med(short)) / (T1 - T0)
    res["setup_seconds"] = med(short) - T0 * res["step_seconds"]  # the column norms, the sweep of b, the uploads, the results
    parts = d.ctx.bench_fsbl(max(calls, 5))
    res["parts_ms"] = parts
    res["parts_ms_sum"] = sum(parts.values())
    esz = 4 if dtype == "float32" else 8
    model = {"score_ms": 6 * 8 * N, "colgemv_ms": 8 * M * M, "rank1_ms": 16 * M * M, "sweep_ms": esz * M * N}
    res["model_bytes"] = model  # the N-pass: alpha, S, Q, w read, S, Q written; C^-1 read once, then read and written; A read once
    res["fraction_of_hbm_peak"] = {k: model[k] / (parts[k] * 1e-3) / HBM_PEAK for k in model}
    d.close()
    return res


def torch_step(At64, y, state):
    """one pass of fsbl on (alpha, Ci, S, Q), Float64 on the card: (action, i)"""
    import torch
    alpha, Ci, S, Q = state
    inf = float("inf")
    active = alpha < inf
    f = torch.where(active, alpha / (alpha - S), torch.ones_like(S))
    s, q = S * f, Q * f
    relevant = s < q * q
    astar = torch.where(relevant, s * s / (q * q - s), torch.full_like(S, inf))
    d = 1.0 / astar - 1.0 / alpha
    add = (Q * Q - S) / S + torch.log(S) - torch.log(Q * Q)
    dele = Q * Q / (S - alpha) - torch.log(1.0 - S / alpha)
    upd = Q * Q / (S + 1.0 / d) - torch.log(torch.clamp(1.0 + S * d, min=0.0))
    val = torch.zeros_like(S)
    val = torch.where(~active & relevant, add, val)
    val = torch.where(active & ~relevant, dele, val)
    val = torch.where(active & relevant, upd, val)
    i = int(torch.argmax(val))
    if not float(val[i]) > 0:
        return 0, i
    a, an = float(alpha[i]), float(astar[i])
    if a == inf:
        act, gam, alpha[i] = 1, 1.0 / an, an
    elif an == inf:
        act, gam, alpha[i] = 2, -1.0 / a, inf
    else:
        act, gam, alpha[i] = 3, 1.0 / an - 1.0 / a, an
    v = Ci @ At64[i]
    den = 1.0 / gam + float(S[i])
    Ci.sub_(torch.outer(v, v) / den)
    w = At64 @ v
    Qi = float(Q[i])
    S.sub_(w * w / den)
    Q.sub_(w * Qi / den)
    return act, i


def mode_torch(M, N, dtype, calls):
    import torch
    cs = load()
    At, S_, y = make_inputs(M, N, dtype)
    d = cs.Dictionary(At)
    At64 = At.to(torch.float64)  # (the restatement keeps a Float64 copy: 2 GiB at 4096 x 65536, where the library reads the Float32 one)
    res = {"mode": "torch", "shape": [M, N, dtype]}
    x = torch.empty(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    info = d.ctx.fsbl_device(y, SIGMA ** 2, x, maxiter=T1, history_cap=T1)
    s2 = SIGMA ** 2
    state = [torch.full((N,), float("inf"), dtype=torch.float64, device="cuda"), torch.eye(M, dtype=torch.float64, device="cuda") / s2,
             (At64 * At64).sum(dim=1) / s2, (At64 @ y) / s2]
    hist, secs = [], []
    for _ in range(T1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        act, i = torch_step(At64, y, state)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        hist.append((act, i))
    alpha, _, _, Q = state
    xt = torch.where(alpha < float("inf"), Q / alpha, torch.zeros_like(Q))
    res["torch_step_seconds"] = secs
    res["torch_step_seconds_median"] = med(secs[T0:])
    res["library_history_is_torchs"] = info["history"] == hist
    res["library_against_torch_max_abs_diff_of_x"] = float((x - xt).abs().max())
    res["max_abs_x"] = float(xt.abs().max())
    d.close()
    return res


def mode_solve(M, N, dtype):
    import torch
    cs = load()
    At, S, y = make_inputs(M, N, dtype)
    d = cs.Dictionary(At)
    x = torch.empty(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d.ctx.fsbl_device(y, SIGMA ** 2, x, maxiter=2)  # warm-up
    res = {"mode": "solve", "shape": [M, N, dtype], "planted": int(S.numel())}
    for solver in ("fsbl", "rmps"):
        t0 = time.perf_counter()
        caps = {"maxiter": 1000} if solver == "fsbl" else {"maxiter": 8}  # (passes; outer iterations)
        info = getattr(d.ctx, solver + "_device")(y, SIGMA ** 2, x, history_cap=4 * N, **caps)
        secs = time.perf_counter() - t0
        found = torch.nonzero(x.abs() > SIGMA).flatten()
        steps = len(info["history"])
        res[solver] = {"caps": caps, "iterations": info["iterations"], "steps": steps, "deletions": sum(a == 2 for a, _ in info["history"]),
                       "converged": info["converged"], "solve_seconds": secs, "seconds_per_step": secs / max(steps, 1),
                       "support_is_planted": bool(torch.equal(found, S)), "entries_above_sigma": int(found.numel()),
                       "nonzeros": int(torch.count_nonzero(x))}
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
    ap.add_argument("--mode", choices=("step", "torch", "solve", "all"), default="step")
    ap.add_argument("--f64", action="store_true", help="2048 x 32768 Float64 instead of 4096 x 65536 Float32")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    M, N, dtype = SHAPES["f64" if a.f64 else "f32"]
    if a.mode == "step":
        print(json.dumps(mode_step(M, N, dtype, a.calls)))
    elif a.mode == "torch":
        print(json.dumps(mode_torch(M, N, dtype, a.calls)))
    elif a.mode == "solve":
        print(json.dumps(mode_solve(M, N, dtype)))
    else:
        res = {"sigma": SIGMA, "hbm_peak_bytes_per_s": HBM_PEAK}

        def save():
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)

        for size, flag, limit in (("f64", ["--f64"], 150), ("f32", [], 200)):
            for mode in ("step", "torch", "solve"):
                res[f"{mode}_{size}"] = child(["--mode", mode, "--calls", str(a.calls)] + flag, limit)
                if mode == "step":
                    res["measured_on"] = res[f"{mode}_{size}"]["device"]
                save()
                print(f"{mode}_{size}", json.dumps({u: v for u, v in res[f"{mode}_{size}"].items() if not isinstance(v, list)}), flush=True)


if __name__ == "__main__":
    main()
