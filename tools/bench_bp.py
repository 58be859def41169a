"""csmp_bp at the benchmark's shape (4096 x 65536 Float32, 20 signals of k = 64 planted atoms).

    python tools/bench_bp.py --mode rowgram        # k_rowgram + its reduction (csmp_bp_rowgram) against torch's Float64 A64 @ A64.T
    python tools/bench_bp.py --mode solve          # the factorisation, then iterations and wall time of the 20 solves to tol = 1e-8
    python tools/bench_bp.py --mode torch          # the same ADMM written with torch Float64 matrices (time yardstick)
    python tools/bench_bp.py --mode once           # one factorisation and 64 iterations: the program a kernel trace is taken of
    python tools/bench_bp.py --mode shapes         # k_rowgram at M = 256 .. 8192, N = 65536: where the column split stops filling the card
    python tools/bench_bp.py --mode all [--out profiles/r15_bp.json]

all runs every step in a fresh child process under a time limit of its own and stops at the first that fails, and adds one
`rocprofv3 --kernel-trace --stats` run of `--mode once` in a process of its own: one iteration split into solve (k_bp_gemv), sweep,
update and axpy, and the kernels of the factorisation.  Flop count of G = A Aᵀ: 2 M² N for both sides (k_rowgram computes the upper
tiles only, half of it).  Needs a GPU; there is no fallback."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, K, NSIG = 4096, 65536, 64, 20


def load():
    sys.path.insert(0, HERE)
    from csmp_pkg import load as ld
    return ld()


def make_inputs(m=M, n=N, nsig=NSIG):
    """unit-norm Gaussian atoms generated on the device (rounded to Float32 once), nsig planted ±1 signals on K atoms, b = A x exactly
    in Float64"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(15)
    At = torch.randn((n, m), generator=g, device="cuda", dtype=torch.float32)
    At /= At.norm(dim=1, keepdim=True)
    B = torch.zeros((nsig, m), dtype=torch.float64, device="cuda")
    for s in range(nsig):
        S = torch.randperm(n, generator=g, device="cuda")[:K]
        v = torch.where(torch.rand(K, generator=g, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
        B[s] = v @ At[S].to(torch.float64)
    At = At.contiguous()
    torch.cuda.synchronize()  # (the library works on a stream of its own: the inputs have to be complete before it reads them)
    return At, B


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def rowgram_row(cs, m, n, reps=3):
    import torch
    At, _ = make_inputs(m, n, 0)
    d = cs.Dictionary(At)
    G = d.ctx.bp_rowgram(device=True)  # warm-up: code objects
    ours = timed(lambda: d.ctx.bp_rowgram(device=True), reps)
    d.close()
    free0 = torch.cuda.mem_get_info()[0]
    A64 = At.to(torch.float64)
    copy_bytes = free0 - torch.cuda.mem_get_info()[0]
    ref = A64.T @ A64
    theirs = timed(lambda: A64.T @ A64, reps)
    diff = float((G - ref).abs().max())
    flop = 2.0 * m * m * n
    mo, mt = sorted(ours)[reps // 2], sorted(theirs)[reps // 2]
    return {"M": m, "N": n, "rowgram_call_s": ours, "torch_f64_gemm_s": theirs, "rowgram_tflops": flop / mo / 1e12, "torch_tflops": flop / mt / 1e12,
            "torch_promoted_copy_bytes": int(copy_bytes), "max_abs_diff": diff}


def mode_rowgram():
    cs = load()
    out = rowgram_row(cs, M, N)
    out["mode"] = "rowgram"
    return out


def mode_shapes():
    cs = load()
    return {"mode": "shapes", "rows": [rowgram_row(cs, m, N) for m in (256, 512, 1024, 2048, 4096, 8192)]}


def mode_solve(once=False):
    import torch
    cs = load()
    At, B = make_inputs()
    d = cs.Dictionary(At)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    t0 = time.perf_counter()
    info = d.ctx.bp_device(B[0], 1.0, x, maxiter=0)  # forms and factorises A Aᵀ, no iteration
    t_factor = time.perf_counter() - t0
    assert info["factored"]
    out = {"mode": "once" if once else "solve", "device": d.ctx.device_info()[0], "factor_call_s": t_factor, "rows": []}
    d.ctx.bp_device(B[0], 1.0, x, maxiter=64)  # warm-up (and the traced iterations of --mode once)
    if not once:
        sweep_ms = sorted(d.ctx.bench_sweep(0, 50) for _ in range(3))[1]
        out["sweep_ms"] = sweep_ms
        for s in range(NSIG):
            t0 = time.perf_counter()
            info = d.ctx.bp_device(B[s], 1.0, x)  # (returns with the work done)
            dt = time.perf_counter() - t0
            out["rows"].append({"signal": s, "seconds": dt, "iterations": info["iterations"], "converged": info["converged"],
                                "resnorm": info["resnorm"], "nnz": int(torch.count_nonzero(x).item()),
                                "ms_per_iteration": 1e3 * dt / max(info["iterations"], 1)})
        ms = sorted(r["ms_per_iteration"] for r in out["rows"])[NSIG // 2]
        out["ms_per_iteration_median"] = ms
        out["iteration_over_sweep"] = ms / sweep_ms
        out["seconds_total"] = sum(r["seconds"] for r in out["rows"])
    d.close()
    return out


def mode_torch(nsig=3, maxiter=16384, tol=1e-8, check_every=32):
    """the textbook iteration on torch Float64 tensors: x = Π(z − u), z⁺ = shrink(x + u, 1/ρ), u⁺ = u + x − z⁺ with a Cholesky of A Aᵀ"""
    import torch
    At, B = make_inputs()
    A64 = At.to(torch.float64)  # (N, M): rows are atoms
    t0 = time.perf_counter()
    L = torch.linalg.cholesky(A64.T @ A64)
    torch.cuda.synchronize()
    out = {"mode": "torch", "factor_s": time.perf_counter() - t0, "rows": []}
    for s in range(nsig):
        b = B[s]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z = torch.zeros(N, dtype=torch.float64, device="cuda")
        u = torch.zeros_like(z)
        it, ok = 0, False
        while it < maxiter and not ok:
            for _ in range(check_every):
                v = z - u
                y = torch.cholesky_solve((v @ A64 - b)[:, None], L)[:, 0]
                xx = v - A64 @ y
                t = xx + u
                zn = torch.sign(t) * torch.clamp(t.abs() - 1.0, min=0.0)
                un = t - zn
                prim, dual = (un - u).norm(), (zn - z).norm()
                z, u = zn, un
                it += 1
            ok = bool(prim < tol) and bool(dual < tol)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["rows"].append({"signal": s, "seconds": dt, "iterations": it, "converged": ok, "ms_per_iteration": 1e3 * dt / it,
                            "nnz": int(torch.count_nonzero(z).item())})
    return out


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


KERNELS = ("k_rowgram_reduce", "k_rowgram", "k_bp_assemble", "k_bp_transpose", "k_chol_row", "k_chol_step", "k_bp_gemv", "k_bp_update", "k_bp_pq",
           "k_bp_fold", "k_bp_start", "k_ista_axpy", "k_ista_resum", "k_sweep")


def trace(outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, mean_us, total_ms}}"""
    os.makedirs(outdir, exist_ok=True)
    child(["--mode", "once"], limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
    kernels = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            short = next((k for k in KERNELS if k in name), None)
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
    ap.add_argument("--mode", choices=("rowgram", "solve", "torch", "once", "shapes", "all"), default="solve")
    ap.add_argument("--out")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "bp_trace"), help="where the kernel trace is written")
    a = ap.parse_args()
    if a.mode == "rowgram":
        print(json.dumps(mode_rowgram()))
    elif a.mode == "shapes":
        print(json.dumps(mode_shapes()))
    elif a.mode in ("solve", "once"):
        print(json.dumps(mode_solve(once=a.mode == "once")))
    elif a.mode == "torch":
        print(json.dumps(mode_torch()))
    else:
        res = {"shape": [M, N, "float32"], "signals": NSIG, "k": K}

        def save():
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)

        for key, args, limit in (("rowgram", ["--mode", "rowgram"], 240), ("solve", ["--mode", "solve"], 300), ("shapes", ["--mode", "shapes"], 300),
                                 ("torch_float64_admm", ["--mode", "torch"], 300)):
            res[key] = child(args, limit)
            save()
        res["kernel_trace_of_one_factorisation_and_64_iterations"] = tr = trace(a.trace_dir, 300)
        g = tr.get("k_rowgram")
        if g:
            res["k_rowgram_kernel_tflops"] = 2.0 * M * M * N / (g["mean_us"] * 1e-6) / 1e12
        it = {k: tr[k]["total_ms"] / 64 * 1e3 for k in ("k_bp_gemv", "k_sweep", "k_bp_update", "k_ista_axpy", "k_ista_resum", "k_bp_pq") if k in tr}
        res["iteration_split_us"] = it
        res["factorisation_kernels_ms"] = {k: tr[k]["total_ms"] for k in ("k_rowgram", "k_rowgram_reduce", "k_bp_assemble", "k_chol_row", "k_chol_step",
                                                                            "k_bp_transpose") if k in tr}
        save()
        print(json.dumps({k: res.get(k) for k in ("k_rowgram_kernel_tflops", "iteration_split_us", "factorisation_kernels_ms")}))
        print(json.dumps({k: v for k, v in res["solve"].items() if k != "rows"}))
        print(json.dumps({k: v for k, v in res["rowgram"].items()}))
        for r in res["shapes"]["rows"]:
            print("M", r["M"], f'rowgram {r["rowgram_tflops"]:.1f} TFLOP/s  torch {r["torch_tflops"]:.1f} TFLOP/s')
        for r in res["torch_float64_admm"]["rows"]:
            print("torch", r)


if __name__ == "__main__":
    main()
