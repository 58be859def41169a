"""csmp_ista at the benchmark's shape (4096 x 65536 Float32): ISTA and FISTA in two regimes chosen by λ -- sparse iterates (λ = 1.6:
the non-zero count stays near the planted 256) and dense iterates (λ = 1e-3: more than N/2 atoms alive).

    python tools/bench_ista.py --mode ista                 # this tree: iterations/s of the four (regime, method) pairs
    python tools/bench_ista.py --mode sweep [--root D]     # the stand-alone product sweep (csmp_bench_sweep) of a built checkout D
    python tools/bench_ista.py --mode torch                # the loop a PyTorch user writes on the Float32 tensor (time yardstick only)
    python tools/bench_ista.py --mode once --regime dense  # one call per method: the program a kernel trace is taken of
    python tools/bench_ista.py --mode all --baseline-root D [--out profiles/r11_ista.json]

all runs every step in a fresh child process under a time limit of its own and stops at the first that fails: the sweep on the
baseline checkout D (the parent commit, built) and on this tree, the four pairs, the torch loop, and one
`rocprofv3 --kernel-trace --stats` run per regime in a process of its own.  It records the sparse regime's time per iteration as a
ratio to the baseline's sweep, and the dense regime's axpy rate (bytes of A the list's columns hold, over the kernel's mean time)
as a ratio to the sweep's rate.  Needs a GPU; there is no fallback."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, K = 4096, 65536, 256
REGIMES = {"sparse": 1.6, "dense": 1e-3}


def make_inputs():
    """unit-norm Gaussian atoms generated on the device, a planted ±1 signal on 256 atoms with 5e-3 noise, stepsize = 0.45 / ‖A‖₂²
    (power iteration in Float64)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(11)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    A32 = At.to(torch.float32).contiguous()
    S = torch.randperm(N, generator=g, device="cuda")[:K]
    xs = torch.zeros(N, dtype=torch.float64, device="cuda")
    xs[S] = torch.where(torch.rand(K, generator=g, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
    At = A32.to(torch.float64)
    b = (xs @ At + 5e-3 * torch.randn(M, generator=g, device="cuda", dtype=torch.float64)).to(torch.float32)
    v = torch.randn(N, generator=g, device="cuda", dtype=torch.float64)
    for _ in range(40):
        v = At @ (v @ At)
        s = v.norm()
        v /= s
    return A32, b, 0.45 / float(s)


def load(root):
    sys.path.insert(0, root)
    from csmp_pkg import load as ld
    return ld()


def mode_sweep(root):
    import torch
    cs = load(root)
    A32, _, _ = make_inputs()
    d = cs.Dictionary(A32)
    d.ctx.bench_sweep(0, 20)
    ms = [d.ctx.bench_sweep(0, 50) for _ in range(3)]
    out = {"mode": "sweep", "root": os.path.basename(os.path.abspath(root)), "device": d.ctx.device_info()[0], "sweep_ms": ms,
           "sweep_ms_median": sorted(ms)[1], "bytes": M * N * 4}
    out["bytes_per_s"] = out["bytes"] / (out["sweep_ms_median"] * 1e-3)
    d.close()
    return out


def mode_ista(root, iters, calls, regimes, once=False):
    import torch
    cs = load(root)
    A32, b, alpha = make_inputs()
    d = cs.Dictionary(A32)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    out = {"mode": "once" if once else "ista", "iters": iters, "stepsize": alpha, "rows": []}
    for regime in regimes:
        for accel in (False, True):
            d.ctx.ista_device(b, REGIMES[regime], x, maxiter=8, stepsize=alpha, accel=accel)  # warm-up: buffers, code objects
            times = []
            for _ in range(1 if once else calls):
                t0 = time.perf_counter()
                rn = d.ctx.ista_device(b, REGIMES[regime], x, maxiter=iters, stepsize=alpha, accel=accel)  # (returns with the work done)
                times.append(time.perf_counter() - t0)
            med = sorted(times)[len(times) // 2]
            out["rows"].append({"regime": regime, "lambda": REGIMES[regime], "method": "fista" if accel else "ista", "seconds": times,
                                "iterations_per_s": iters / med, "ms_per_iteration": 1e3 * med / iters,
                                "nnz_of_result": int(torch.count_nonzero(x).item()), "resnorm": rn})
    d.close()
    return out


def mode_torch(iters, calls):
    """what a PyTorch-ROCm user writes today: Float32 arithmetic on the (N, M) tensor -- a TIME yardstick, not a parity one"""
    import torch
    A32, b, alpha = make_inputs()
    out = {"mode": "torch", "iters": iters, "rows": []}
    for regime, lam in REGIMES.items():
        for accel in (False, True):
            times = []
            for _ in range(calls + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x = torch.zeros(N, dtype=torch.float32, device="cuda")
                y, t = x.clone(), 1.0
                for _ in range(iters):
                    g = A32 @ (b - y @ A32)
                    u = y + 2 * alpha * g
                    xn = torch.sign(u) * torch.clamp(u.abs() - lam * alpha, min=0.0)
                    tn = (1.0 + (1.0 + 4.0 * t * t) ** 0.5) / 2.0
                    y = xn + ((t - 1.0) / tn) * (xn - x) if accel else xn
                    x, t = xn, tn
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            times = times[1:]  # (the first is the warm-up)
            med = sorted(times)[len(times) // 2]
            out["rows"].append({"regime": regime, "method": "fista" if accel else "ista", "seconds": times, "iterations_per_s": iters / med,
                                "ms_per_iteration": 1e3 * med / iters, "nnz_of_result": int(torch.count_nonzero(x).item())})
    return out


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def trace(regime, iters, outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, mean_us}}"""
    os.makedirs(outdir, exist_ok=True)
    child(["--mode", "once", "--regime", regime, "--iters", str(iters)], limit,
          prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
    kernels = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            short = next((k for k in ("k_ista_axpy", "k_ista_resum", "k_ista_update", "k_sweep", "k_norm2", "k_init") if k in name), None)
            if short:
                e = kernels.setdefault(short, {"calls": 0, "total_ns": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += float(row["TotalDurationNs"])
    for e in kernels.values():
        e["mean_us"] = e["total_ns"] / max(e["calls"], 1) / 1e3
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("ista", "sweep", "torch", "once", "all"), default="ista")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="all: a built checkout of the parent commit")
    ap.add_argument("--regime", choices=tuple(REGIMES) + ("both",), default="both")
    ap.add_argument("--iters", type=int, default=256)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "ista_trace"), help="where the kernel traces are written")
    a = ap.parse_args()
    regimes = tuple(REGIMES) if a.regime == "both" else (a.regime,)
    if a.mode == "sweep":
        print(json.dumps(mode_sweep(a.root)))
    elif a.mode in ("ista", "once"):
        print(json.dumps(mode_ista(a.root, a.iters, a.calls, regimes, once=a.mode == "once")))
    elif a.mode == "torch":
        print(json.dumps(mode_torch(a.iters, a.calls)))
    else:
        if not a.baseline_root:
            raise SystemExit("--mode all needs --baseline-root")
        base = child(["--mode", "sweep", "--root", a.baseline_root], 240)
        here = child(["--mode", "sweep"], 240)
        ista = child(["--mode", "ista", "--iters", str(a.iters), "--calls", str(a.calls)], 420)
        torch_rows = child(["--mode", "torch", "--iters", str(a.iters), "--calls", str(a.calls)], 300)
        traces = {r: trace(r, 64, os.path.join(a.trace_dir, r), 300) for r in REGIMES}
        row = {(r["regime"], r["method"]): r for r in ista["rows"]}
        res = {"shape": [M, N, "float32"], "iters": a.iters, "regimes": REGIMES, "measured_on": here["device"],
               "baseline_sweep": base, "sweep": here, "ista": ista, "torch_float32_loop": torch_rows, "kernel_trace": traces}
        sweep_ms = base["sweep_ms_median"]
        res["sparse_ms_per_iteration_over_baseline_sweep_ms"] = {m: row[("sparse", m)]["ms_per_iteration"] / sweep_ms for m in ("ista", "fista")}
        ax = traces["dense"].get("k_ista_axpy")
        if ax:  # bytes: the columns of the result's non-zeros (the list of the last iterations; λ = 1e-3 keeps nearly every atom alive)
            nbytes = row[("dense", "ista")]["nnz_of_result"] * M * 4
            res["dense_axpy"] = {"bytes": nbytes, "mean_us": ax["mean_us"], "bytes_per_s": nbytes / (ax["mean_us"] * 1e-6)}
            res["dense_axpy_rate_over_sweep_rate"] = res["dense_axpy"]["bytes_per_s"] / here["bytes_per_s"]
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps({k: res.get(k) for k in ("sparse_ms_per_iteration_over_baseline_sweep_ms", "dense_axpy", "dense_axpy_rate_over_sweep_rate")}))
        for r in ista["rows"] + torch_rows["rows"]:
            print(r["regime"], r["method"], f'{r["ms_per_iteration"]:.4f} ms/iteration', r["nnz_of_result"])
        print(json.dumps(traces))


if __name__ == "__main__":
    main()
