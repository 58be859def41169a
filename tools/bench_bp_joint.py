"""csmp_bp_joint against csmp_bp_batch on the same B, at the benchmark's shape (4096 x 65536 Float32, tools/bench_ista.py's dictionary):
64 planted ROWS shared by all columns, amplitudes ±(0.5 … 1.5), noiseless (B = A X in Float64), ρ = 1, tol = 1e-8, check_every = 32, at 8 / 16 / 64 columns.
The two solve different problems (one support and one stopping rule for all columns against one of each per column): what is
compared is the cost of an iteration for the same number of columns, the iterations to convergence, and the rows found.

    python tools/bench_bp_joint.py --mode joint            # this tree: csmp_bp_joint
    python tools/bench_bp_joint.py --mode batch [--root D] # csmp_bp_batch on the same B (D: another built checkout)
    python tools/bench_bp_joint.py --mode once --side joint   # one call of eight columns, 32 iterations: for a kernel trace
    python tools/bench_bp_joint.py --mode ab --baseline-root D [--rounds 2] [--out profiles/r26_bp_joint.json] [--trace]

ab alternates fresh child processes -- csmp_bp_batch on the baseline checkout D (the parent commit, built), csmp_bp_joint on this
tree --, every child under a time limit of its own, and stops at the first that fails.  Per nsig: the time of a whole solve by the
host clock around the call (device pointers in and out; both return with the work done; the factorisation is done before), the
iterations, and the time per COLUMN-iteration -- seconds over nsig x iterations for the joint call, over the sum of the columns'
iterations for the batch -- times eight: the cost of a step of eight columns.  The median of each side, their ratio and each side's
spread between all its readings ((max - min) / median).  Nothing is asserted about the times.  --trace adds one
`rocprofv3 --kernel-trace --stats` run of `--mode once` per side, each in a process of its own: the kernels' mean times and the
launches per iteration.  Needs a GPU; there is no fallback."""
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
from bench_ista import M, N, load, make_inputs  # noqa: E402
K = 64
NSIGS = (8, 16, 64)
RHO, TOL, CHECK_EVERY, MAXITER = 1.0, 1e-8, 32, 8192
ONCE_ITERS, ONCE_COLS = 32, 8


def make_signals(nsig):
    """bench_ista.py's dictionary; B (nsig, M) = the same K rows planted in every column, in Float64: B = A X exactly as far as Float64
    goes (rounded to Float32, B is 1e-7 away from the span of the planted atoms, and the equality constraint then asks for a dense
    correction that neither solver reaches in 65 536 iterations); the rows"""
    import torch
    A32, _, _ = make_inputs()
    g = torch.Generator(device="cuda").manual_seed(2600)
    S = torch.randperm(N, generator=g, device="cuda")[:K]
    sign = torch.where(torch.rand((nsig, K), generator=g, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
    amp = sign * (0.5 + torch.rand((nsig, K), generator=g, device="cuda", dtype=torch.float64))
    B = amp @ A32[S].to(torch.float64)
    return A32, B.contiguous(), torch.sort(S).values


def measure(mode, root, calls, nsigs, maxiter):
    import torch
    cs = load(root)
    A32, B, S = make_signals(max(nsigs))
    d = cs.Dictionary(A32)
    out = {"mode": mode, "root": os.path.basename(os.path.abspath(root)), "calls": calls, "device": d.ctx.device_info()[0],
           "sweep_config": d.ctx.sweep_config(), "rows": []}
    solve = d.ctx.bp_joint_device if mode == "joint" else d.ctx.bp_batch_device
    kw = dict(rho=RHO, tol=TOL, check_every=CHECK_EVERY)
    for nsig in nsigs:
        X = torch.zeros((nsig, N), dtype=torch.float64, device="cuda")
        Bt, Xt = B[:nsig].T, X.T  # columns = signals, leading dimensions M and N
        solve(Bt, 1.0, Xt, maxiter=4, **kw)  # warm-up: the factor (the first call), buffers, code objects
        times, res = [], None
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = solve(Bt, 1.0, Xt, maxiter=maxiter, **kw)
            times.append(time.perf_counter() - t0)
        live = (X != 0).any(dim=0)
        row = {"nsig": nsig, "seconds": times, "resnorm_max": float(max(res["resnorm"])),
               "rows_with_a_nonzero": int(live.sum()), "planted_rows_found": int(live[S].sum()), "planted_rows": K}
        if mode == "joint":
            col_its = nsig * res["iterations"]
            row.update(iterations=res["iterations"], converged=res["converged"], rows_of_the_result=res["rows"])
        else:
            its = [int(v) for v in res["iterations"]]
            col_its = sum(its)
            nnz = torch.count_nonzero(X, dim=1)
            row.update(iterations_min_median_max=[min(its), sorted(its)[len(its) // 2], max(its)], converged=int(res["converged"].sum()),
                       nnz_of_results_min_max=[int(nnz.min()), int(nnz.max())])
        row["column_iterations"] = col_its
        row["us_per_step_of_8_columns"] = [8e6 * t / max(col_its, 1) for t in times]
        out["rows"].append(row)
    d.close()
    return out


def once(root, side):
    import torch
    cs = load(root)
    A32, B, _ = make_signals(ONCE_COLS)
    d = cs.Dictionary(A32)
    X = torch.zeros((ONCE_COLS, N), dtype=torch.float64, device="cuda")
    solve = d.ctx.bp_joint_device if side == "joint" else d.ctx.bp_batch_device
    info = solve(B.T, 1.0, X.T, rho=RHO, maxiter=ONCE_ITERS, tol=TOL, check_every=CHECK_EVERY)
    d.close()
    return {"mode": "once", "side": side, "columns": ONCE_COLS, "iterations": ONCE_ITERS,
            "iterations_done": info["iterations"] if side == "joint" else [int(v) for v in info["iterations"]]}


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


KERNELS = ("k_sweep_wide", "k_sweep_multi", "k_sweep", "k_jbp_update", "k_jbp_pq", "k_jbp_start", "k_jbp_norm2", "k_jista_axpy", "k_jista_resum",
           "k_somp_init", "k_bp_gemm", "k_bp_update_group", "k_ista_axpy_group", "k_ista_resum_group", "k_bp_pq_group", "k_bp_fold", "k_bp_start",
           "k_land_multi", "k_norm2", "k_init")
STEP = {"joint": ("k_bp_gemm", "k_sweep_wide", "k_jbp_update", "k_jista_axpy", "k_jista_resum", "k_jbp_pq"),
        "batch": ("k_bp_gemm", "k_sweep_wide", "k_bp_update_group", "k_ista_axpy_group", "k_ista_resum_group", "k_bp_pq_group")}


def trace(root, side, outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, mean_us, total_ms}}; the
    factorisation's kernels (k_rowgram, k_chol_*) are part of the run and are left out of the table"""
    os.makedirs(outdir, exist_ok=True)
    info = child(["--mode", "once", "--side", side, "--root", root], limit,
                 prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
    kernels = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            short = next((k for k in KERNELS if k in name), None)  # (the longer names come first)
            if short:
                e = kernels.setdefault(short, {"calls": 0, "total_ns": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += float(row["TotalDurationNs"])
    for e in kernels.values():
        e["mean_us"] = e["total_ns"] / max(e["calls"], 1) / 1e3
        e["total_ms"] = e.pop("total_ns") / 1e6
    step = {k: {"launches": kernels[k]["calls"] / ONCE_ITERS, "us": kernels[k]["total_ms"] * 1e3 / ONCE_ITERS} for k in STEP[side] if k in kernels}
    return {"program": info, "kernels": kernels, "per_iteration": step, "kernel_us_per_iteration": sum(v["us"] for v in step.values())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("joint", "batch", "once", "ab"), default="joint")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="ab: a built checkout of the parent commit")
    ap.add_argument("--side", choices=("joint", "batch"), default="joint", help="once: the call to run")
    ap.add_argument("--maxiter", type=int, default=MAXITER)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nsig", default=",".join(map(str, NSIGS)))
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "bp_joint_trace"))
    ap.add_argument("--out")
    a = ap.parse_args()
    nsigs = tuple(int(x) for x in a.nsig.split(","))
    if a.mode == "once":
        print(json.dumps(once(a.root, a.side)))
        return
    if a.mode != "ab":
        print(json.dumps(measure(a.mode, a.root, a.calls, nsigs, a.maxiter)))
        return
    if not a.baseline_root:
        raise SystemExit("--mode ab needs --baseline-root")
    if a.rounds < 2:
        raise SystemExit("--mode ab needs at least two rounds: the spread of each side is part of the result")
    res = {"shape": [M, N, "float32"], "signals": f"{K} planted rows shared by all columns, amplitudes ±(0.5 … 1.5), noiseless (B in Float64)",
           "rho": RHO, "tol": TOL, "check_every": CHECK_EVERY, "maxiter": a.maxiter,
           "baseline": "the parent commit: csmp_bp_batch on the same B", "runs": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    common = ["--maxiter", str(a.maxiter), "--calls", str(a.calls), "--nsig", a.nsig]
    for _ in range(a.rounds):  # builds alternated in one session
        res["runs"].append(child(["--mode", "batch", "--root", a.baseline_root] + common, a.limit))
        save()
        res["runs"].append(child(["--mode", "joint", "--root", a.root] + common, a.limit))
        save()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    table = []
    for nsig in nsigs:
        rows = {m: [row for r in res["runs"] if r["mode"] == m for row in r["rows"] if row["nsig"] == nsig] for m in ("batch", "joint")}
        t = {m: [x for row in rows[m] for x in row["us_per_step_of_8_columns"]] for m in rows}
        s = {m: [x for row in rows[m] for x in row["seconds"]] for m in rows}
        jb, bb = rows["joint"][-1], rows["batch"][-1]
        table.append({"nsig": nsig, "batch_us_per_step_of_8": med(t["batch"]), "batch_spread": spread(t["batch"]),
                      "joint_us_per_step_of_8": med(t["joint"]), "joint_spread": spread(t["joint"]),
                      "joint_over_batch_step": med(t["joint"]) / med(t["batch"]),
                      "batch_seconds": med(s["batch"]), "joint_seconds": med(s["joint"]),
                      "batch_iterations_min_median_max": bb["iterations_min_median_max"], "batch_converged": bb["converged"],
                      "joint_iterations": jb["iterations"], "joint_converged": jb["converged"],
                      "batch_planted_rows_found": bb["planted_rows_found"], "batch_rows_with_a_nonzero": bb["rows_with_a_nonzero"],
                      "joint_planted_rows_found": jb["planted_rows_found"], "joint_rows": jb["rows_of_the_result"]})
    res["table"] = table
    save()
    if a.trace:
        key = f"kernel_trace_of_{ONCE_ITERS}_iterations_of_{ONCE_COLS}_columns"
        res[key] = {"joint": trace(a.root, "joint", os.path.join(a.trace_dir, "joint"), a.limit),
                    "batch": trace(a.baseline_root, "batch", os.path.join(a.trace_dir, "batch"), a.limit)}
        save()
        for side, t in res[key].items():
            print(side, json.dumps({k: [v["launches"], round(v["us"], 1)] for k, v in t["per_iteration"].items()}),
                  round(t["kernel_us_per_iteration"], 1))
    for t in table:
        print(json.dumps(t))


if __name__ == "__main__":
    main()
