"""csmp_bpd at the benchmark's shape (4096 x 65536 Float32, noisy signals of k = 64 planted atoms, sigma = 1e-2 a row: delta = sigma sqrt(M)).

    python tools/bench_bpd.py --mode iter          # the factorisation, then bpd and bp alternated on ONE context, a fixed number of iterations
                                                   # each: time per iteration of both, their ratio and its run-to-run spread
    python tools/bench_bpd.py --mode solve         # iterations and wall time of the solves to tol = 1e-8 at the default rho
    python tools/bench_bpd.py --mode candes        # one bpd_candes solve (reference defaults: eps = delta, maxiter = 8, min_decrease = 1e-4)
    python tools/bench_bpd.py --mode once          # one factorisation and 64 iterations: the program a kernel trace is taken of
    python tools/bench_bpd.py --mode all [--out profiles/r16_bpd.json]

all runs every step in a fresh child process under a time limit of its own and stops at the first that fails, and adds one
`rocprofv3 --kernel-trace --stats` run of `--mode once` in a process of its own: one iteration split by kernel.  Needs a GPU; there is no
fallback."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_bp as bb  # noqa: E402

M, N, K = bb.M, bb.N, bb.K
NSIG, SIGMA = 4, 1e-2
ITERS, REPS = 2048, 5  # about half a second a reading
NEVER = 1e-300  # a tol no residual passes: the call runs exactly maxiter iterations


def make_inputs(nsig=NSIG):
    import torch
    At, B = bb.make_inputs(M, N, nsig)
    g = torch.Generator(device="cuda").manual_seed(16)
    B += SIGMA * torch.randn(B.shape, generator=g, device="cuda", dtype=torch.float64)
    torch.cuda.synchronize()
    return At, B, SIGMA * M ** 0.5


def spread(v):
    return (max(v) - min(v)) / sorted(v)[len(v) // 2]


def mode_iter(once=False):
    import torch
    cs = bb.load()
    At, B, delta = make_inputs(1)
    rho = cs._lib.BPD_RHO
    d = cs.Dictionary(At)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    t0 = time.perf_counter()
    info = d.ctx.bpd_device(B[0], delta, 1.0, x, maxiter=0)  # forms A Aᵀ, factorises I + A Aᵀ, no iteration
    t_factor = time.perf_counter() - t0
    assert info["factored"]
    out = {"mode": "once" if once else "iter", "device": d.ctx.device_info()[0], "delta": delta, "rho": rho, "bpd_factor_call_s": t_factor}
    d.ctx.bpd_device(B[0], delta, 1.0, x, rho=rho, maxiter=64, tol=NEVER)  # warm-up (and the traced iterations of --mode once)
    if not once:
        t0 = time.perf_counter()
        assert d.ctx.bp_device(B[0], 1.0, x, maxiter=0)["factored"]
        out["bp_factor_call_s"] = time.perf_counter() - t0
        d.ctx.bp_device(B[0], 1.0, x, maxiter=64, tol=NEVER)
        out["sweep_ms"] = sorted(d.ctx.bench_sweep(0, 50) for _ in range(3))[1]
        bpd_ms, bp_ms, nnz = [], [], {}
        for _ in range(REPS):  # alternated: a drift of the clocks meets both alike
            t0 = time.perf_counter()
            i1 = d.ctx.bpd_device(B[0], delta, 1.0, x, rho=rho, maxiter=ITERS, tol=NEVER)
            bpd_ms.append(1e3 * (time.perf_counter() - t0) / ITERS)
            nnz["bpd"] = int(torch.count_nonzero(x).item())
            t0 = time.perf_counter()
            i2 = d.ctx.bp_device(B[0], 1.0, x, maxiter=ITERS, tol=NEVER)
            bp_ms.append(1e3 * (time.perf_counter() - t0) / ITERS)
            nnz["bp"] = int(torch.count_nonzero(x).item())
            assert i1["iterations"] == i2["iterations"] == ITERS and not i1["factored"] and not i2["factored"]
        ratios = [a / b for a, b in zip(bpd_ms, bp_ms)]
        out.update({"iterations_per_reading": ITERS, "bpd_ms_per_iteration": bpd_ms, "bp_ms_per_iteration": bp_ms, "ratio_bpd_over_bp": ratios,
                    "ratio_median": sorted(ratios)[REPS // 2], "ratio_spread": spread(ratios), "bpd_spread": spread(bpd_ms), "bp_spread": spread(bp_ms),
                    "nnz_of_the_last_iterate": nnz,
                    "note": "the axpy over the non-zeros of z+ is part of an iteration: bp's iterate on noisy data is denser than bpd's"})
    d.close()
    return out


def mode_solve():
    import torch
    cs = bb.load()
    At, B, delta = make_inputs()
    d = cs.Dictionary(At)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    d.ctx.bpd_device(B[0], delta, 1.0, x, maxiter=64)  # factorisation and warm-up
    out = {"mode": "solve", "delta": delta, "rho": cs._lib.BPD_RHO, "tol": 1e-8, "rows": []}
    for s in range(NSIG):
        t0 = time.perf_counter()
        info = d.ctx.bpd_device(B[s], delta, 1.0, x)
        dt = time.perf_counter() - t0
        out["rows"].append({"signal": s, "seconds": dt, "iterations": info["iterations"], "converged": info["converged"], "resnorm": info["resnorm"],
                            "nnz": int(torch.count_nonzero(x).item()), "ms_per_iteration": 1e3 * dt / max(info["iterations"], 1)})
    d.close()
    return out


def mode_candes():
    import torch
    cs = bb.load()
    At, B, delta = make_inputs(1)
    d = cs.Dictionary(At)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    d.ctx.bpd_device(B[0], delta, 1.0, x, maxiter=64)  # factorisation and warm-up
    t0 = time.perf_counter()
    rn, done = d.ctx.bpd_reweighted_device(B[0], delta, "candes", x)
    dt = time.perf_counter() - t0
    d.close()
    return {"mode": "candes", "delta": delta, "eps": delta, "rho": cs._lib.BPD_RHO, "seconds": dt, "solves": done, "resnorm": rn,
            "nnz": int(torch.count_nonzero(x).item())}


KERNELS = ("k_rowgram_reduce", "k_rowgram", "k_bpd_assemble", "k_bp_transpose", "k_chol_row", "k_chol_step", "k_bp_gemv", "k_bp_update", "k_bpd_pq",
           "k_bpd_ball", "k_bpd_fold", "k_bpd_start", "k_ista_axpy", "k_ista_resum", "k_sweep")


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def trace(outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, mean_us, total_ms}}"""
    os.makedirs(outdir, exist_ok=True)
    child(["--mode", "once"], limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
    kernels = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            short = next((k for k in KERNELS if k in row.get("Name", "")), None)
            if short:
                e = kernels.setdefault(short, {"calls": 0, "total_ns": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += float(row["TotalDurationNs"])
    for e in kernels.values():
        e["mean_us"] = e["total_ns"] / max(e["calls"], 1) / 1e3
        e["total_ms"] = e.pop("total_ns") / 1e6
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("iter", "solve", "candes", "once", "all"), default="iter")
    ap.add_argument("--out")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "bpd_trace"), help="where the kernel trace is written")
    a = ap.parse_args()
    if a.mode in ("iter", "once"):
        print(json.dumps(mode_iter(once=a.mode == "once")))
    elif a.mode == "solve":
        print(json.dumps(mode_solve()))
    elif a.mode == "candes":
        print(json.dumps(mode_candes()))
    else:
        res = {"shape": [M, N, "float32"], "k": K, "sigma": SIGMA}

        def save():
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)

        for key, args, limit in (("iter", ["--mode", "iter"], 240), ("solve", ["--mode", "solve"], 240), ("bpd_candes", ["--mode", "candes"], 240)):
            res[key] = child(args, limit)
            save()
        res["kernel_trace_of_one_factorisation_and_64_iterations"] = tr = trace(a.trace_dir, 240)
        res["iteration_split_us"] = {k: tr[k]["total_ms"] / 64 * 1e3 for k in ("k_bp_gemv", "k_sweep", "k_bp_update", "k_ista_axpy", "k_ista_resum",
                                                                                 "k_bpd_pq", "k_bpd_ball") if k in tr}
        save()
        print(json.dumps({k: v for k, v in res["iter"].items()}))
        print(json.dumps(res["iteration_split_us"]))
        for r in res["solve"]["rows"]:
            print("solve", r)
        print(json.dumps(res["bpd_candes"]))


if __name__ == "__main__":
    main()
