"""csmp_ista_joint against csmp_ista_batch on the same B, at the benchmark's shape (4096 x 65536 Float32, tools/bench_ista.py's dictionary
and step size): 256 planted ROWS shared by all columns, amplitudes ±(0.5 … 1.5), 5e-3 noise; ISTA and FISTA with sparse iterates
(λ = 0.2) and dense iterates (λ = 1e-3), 8 / 16 / 64 columns.  The two solve different problems (one support for all columns against
one per column): what is compared is the time of an iteration for the same number of columns.

    python tools/bench_ista_joint.py --mode joint            # this tree: csmp_ista_joint
    python tools/bench_ista_joint.py --mode batch [--root D] # csmp_ista_batch on the same B (D: another built checkout)
    python tools/bench_ista_joint.py --mode once --regime dense   # one joint call and one batch of eight columns, 32 iterations: for a kernel trace
    python tools/bench_ista_joint.py --mode ab --baseline-root D [--rounds 2] [--out profiles/r25_ista_joint.json] [--trace]

ab alternates fresh child processes -- csmp_ista_batch on the baseline checkout D (the parent commit, built), csmp_ista_joint on this
tree --, every child under a time limit of its own, and stops at the first that fails.  Per (regime, method, nsig): the time of one
iteration by the host clock around the call (device pointers in and out; both return with the work done), the median of each side,
their ratio and each side's spread between all its readings ((max - min) / median).  Nothing is asserted about the times.  --trace
adds one `rocprofv3 --kernel-trace --stats` run of `--mode once` per regime, each in a process of its own: the kernels' mean times and
the launches per iteration.  Needs a GPU; there is no fallback."""
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
from bench_ista import K, M, N, load, make_inputs  # noqa: E402
REGIMES = {"sparse": 0.2, "dense": 1e-3}
NSIGS = (8, 16, 64)
ONCE_ITERS, ONCE_COLS = 32, 8


def make_signals(nsig):
    """bench_ista.py's dictionary and step size; B (nsig, M): the same K rows planted in every column"""
    import torch
    A32, _, alpha = make_inputs()
    g = torch.Generator(device="cuda").manual_seed(2500)
    S = torch.randperm(N, generator=g, device="cuda")[:K]
    sign = torch.where(torch.rand((nsig, K), generator=g, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
    amp = sign * (0.5 + torch.rand((nsig, K), generator=g, device="cuda", dtype=torch.float64))
    B = (amp @ A32[S].to(torch.float64) + 5e-3 * torch.randn((nsig, M), generator=g, device="cuda", dtype=torch.float64)).to(torch.float32)
    return A32, B.contiguous(), alpha


def measure(mode, root, iters, calls, nsigs, regimes):
    import torch
    cs = load(root)
    A32, B, alpha = make_signals(max(nsigs))
    d = cs.Dictionary(A32)
    out = {"mode": mode, "root": os.path.basename(os.path.abspath(root)), "iters": iters, "calls": calls, "stepsize": alpha,
           "device": d.ctx.device_info()[0], "sweep_config": d.ctx.sweep_config(), "rows": []}
    solve = d.ctx.ista_joint_device if mode == "joint" else d.ctx.ista_batch_device
    for regime in regimes:
        lam = REGIMES[regime]
        for accel in (False, True):
            for nsig in nsigs:
                X = torch.zeros((nsig, N), dtype=torch.float64, device="cuda")
                Bt, Xt = B[:nsig].T, X.T  # columns = signals, leading dimensions M and N
                solve(Bt, lam, Xt, maxiter=4, stepsize=alpha, accel=accel)  # warm-up: buffers, code objects
                times, res = [], None
                for _ in range(calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = solve(Bt, lam, Xt, maxiter=iters, stepsize=alpha, accel=accel)
                    times.append(time.perf_counter() - t0)
                row = {"regime": regime, "lambda": lam, "method": "fista" if accel else "ista", "nsig": nsig, "seconds": times,
                       "us_per_iteration": [1e6 * t / iters for t in times]}
                if mode == "joint":
                    row["rows_of_the_result"] = res["rows"]
                    row["resnorm_max"] = float(max(res["resnorm"]))
                else:
                    row["nnz_of_results_min_max"] = [int(torch.count_nonzero(X, dim=1).min()), int(torch.count_nonzero(X, dim=1).max())]
                    row["resnorm_max"] = float(max(res))
                out["rows"].append(row)
    d.close()
    return out


def once(root, regime):
    import torch
    cs = load(root)
    A32, B, alpha = make_signals(ONCE_COLS)
    d = cs.Dictionary(A32)
    X = torch.zeros((ONCE_COLS, N), dtype=torch.float64, device="cuda")
    info = d.ctx.ista_joint_device(B.T, REGIMES[regime], X.T, maxiter=ONCE_ITERS, stepsize=alpha)
    d.ctx.ista_batch_device(B.T, REGIMES[regime], X.T, maxiter=ONCE_ITERS, stepsize=alpha)
    nnz = torch.count_nonzero(X, dim=1).tolist()
    d.close()
    return {"mode": "once", "regime": regime, "columns": ONCE_COLS, "iterations": ONCE_ITERS, "rows_of_the_joint_result": info["rows"],
            "nnz_of_the_batch_results": nnz}


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


KERNELS = ("k_sweep_wide", "k_sweep_multi", "k_sweep", "k_jista_update", "k_jista_axpy", "k_jista_resum", "k_jista_norm2", "k_somp_init",
           "k_ista_update_group", "k_ista_update", "k_ista_axpy_group", "k_ista_axpy", "k_ista_resum_group", "k_ista_resum", "k_norm2", "k_init")


def trace(regime, outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, mean_us, total_ms}}"""
    os.makedirs(outdir, exist_ok=True)
    info = child(["--mode", "once", "--regime", regime], limit,
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
    # the joint call's own kernels; the shared pass (k_sweep_wide) serves both calls, one launch per iteration and chunk of eight each
    per_it = {k: kernels[k]["calls"] / ONCE_ITERS for k in ("k_jista_update", "k_jista_axpy", "k_jista_resum") if k in kernels}
    if "k_sweep_wide" in kernels:
        per_it["k_sweep_wide"] = kernels["k_sweep_wide"]["calls"] / (2 * ONCE_ITERS)
    return {"program": info, "kernels": kernels, "launches_per_iteration_of_the_joint_call": per_it}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("joint", "batch", "once", "ab"), default="joint")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="ab: a built checkout of the parent commit")
    ap.add_argument("--regime", choices=tuple(REGIMES) + ("both",), default="both")
    ap.add_argument("--iters", type=int, default=64, help="iterations of every solve")
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nsig", default=",".join(map(str, NSIGS)))
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "ista_joint_trace"))
    ap.add_argument("--out")
    a = ap.parse_args()
    nsigs = tuple(int(x) for x in a.nsig.split(","))
    regimes = tuple(REGIMES) if a.regime == "both" else (a.regime,)
    if a.mode == "once":
        print(json.dumps(once(a.root, regimes[0])))
        return
    if a.mode != "ab":
        print(json.dumps(measure(a.mode, a.root, a.iters, a.calls, nsigs, regimes)))
        return
    if not a.baseline_root:
        raise SystemExit("--mode ab needs --baseline-root")
    if a.rounds < 2:
        raise SystemExit("--mode ab needs at least two rounds: the spread of each side is part of the result")
    res = {"shape": [M, N, "float32"], "signals": "256 planted rows shared by all columns, amplitudes ±(0.5 … 1.5), 5e-3 noise", "regimes": REGIMES,
           "iters": a.iters, "baseline": "the parent commit: csmp_ista_batch on the same B", "runs": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    common = ["--iters", str(a.iters), "--calls", str(a.calls), "--nsig", a.nsig, "--regime", a.regime]
    for _ in range(a.rounds):  # builds alternated in one session
        res["runs"].append(child(["--mode", "batch", "--root", a.baseline_root] + common, a.limit))
        save()
        res["runs"].append(child(["--mode", "joint", "--root", a.root] + common, a.limit))
        save()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    table = []
    for regime in regimes:
        for method in ("ista", "fista"):
            for nsig in nsigs:
                t = {m: [x for r in res["runs"] if r["mode"] == m for row in r["rows"]
                         if (row["regime"], row["method"], row["nsig"]) == (regime, method, nsig) for x in row["us_per_iteration"]]
                     for m in ("batch", "joint")}
                table.append({"regime": regime, "method": method, "nsig": nsig, "batch_us_per_iteration": med(t["batch"]),
                              "batch_spread": spread(t["batch"]), "joint_us_per_iteration": med(t["joint"]), "joint_spread": spread(t["joint"]),
                              "batch_over_joint": med(t["batch"]) / med(t["joint"])})
    res["table"] = table
    save()
    if a.trace:
        key = f"kernel_trace_of_{ONCE_ITERS}_iterations_of_{ONCE_COLS}_columns_joint_then_batch"
        res[key] = {r: trace(r, os.path.join(a.trace_dir, r), a.limit) for r in regimes}
        save()
        for r, t in res[key].items():
            print(r, json.dumps({k: [v["calls"], round(v["mean_us"], 2)] for k, v in t["kernels"].items()}))
    for t in table:
        print(json.dumps(t))


if __name__ == "__main__":
    main()
