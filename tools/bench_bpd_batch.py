"""csmp_bpd_batch against the caller's loop over csmp_bpd, at the benchmark's shape (4096 x 65536 Float32, tools/bench_bpd.py's signals:
k = 64 planted atoms, noise of sigma = 1e-2 a row, delta = sigma sqrt(M), the default rho, tol = 1e-8).

    python tools/bench_bpd_batch.py --mode batch            # this tree: csmp_bpd_batch, nsig in (1, 2, 4, 8, 16)
    python tools/bench_bpd_batch.py --mode loop [--root D]  # the loop of csmp_bpd over the same signals (D: another built checkout)
    python tools/bench_bpd_batch.py --mode once             # one batch of eight signals, 64 iterations: the program a kernel trace is taken of
    python tools/bench_bpd_batch.py --mode ab --baseline-root D [--rounds 2] [--out profiles/r20_bpd_batch.json] [--trace]

ab alternates fresh child processes, one at a time -- the loop on the baseline checkout D (the parent commit, built), the batch on this
tree --, every child under a time limit of its own, and stops at the first that fails.  One factorising call comes first in every child
and stays outside the timings.  Per nsig: signals/s by the host clock around the call (device pointers in and out; both forms return
with the work done), `--calls` calls per child.  Reported: the median of each side, their ratio, and each side's spread between all its
readings ((max - min) / median).  The conditions: at nsig = 8 and 16 the batch beats the loop by more than the larger of the two
spreads; at nsig = 1, where the batch takes the loop's own path, the two are within that spread of each other.
--trace adds one `rocprofv3 --kernel-trace --stats` run of `--mode once` in a process of its own, with no counters in it: a step of eight
members split into k_bp_gemm, the shared pass and the group kernels, beside k_bp_gemv and the single kernels of a loop of the same
iterations.  Needs a GPU; there is no fallback."""
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
from bench_bpd import M, N, NEVER, make_inputs  # noqa: E402
NSIGS = (1, 2, 4, 8, 16)


def setup(root, nsig):
    sys.path.insert(0, root)
    import torch
    from csmp_pkg import load
    cs = load()
    At, B, delta = make_inputs(nsig)
    d = cs.Dictionary(At)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    info = d.ctx.bpd_device(B[0], delta, 1.0, x, maxiter=0)  # forms A Aᵀ and factorises I + A Aᵀ: outside every timing
    assert info["factored"]
    return cs, d, B, delta, x


def measure(mode, root, calls, nsigs):
    import numpy as np
    import torch
    cs, d, B, delta, x = setup(root, max(nsigs))
    out = {"mode": mode, "root": os.path.basename(os.path.abspath(root)), "calls": calls, "device": d.ctx.device_info()[0], "delta": delta,
           "rho": cs._lib.BPD_RHO, "rows": []}
    if mode == "batch":
        out["sweep_config"] = d.ctx.sweep_config()
    d.ctx.bpd_device(B[0], delta, 1.0, x, maxiter=64)  # warm-up: code objects
    for nsig in nsigs:
        row = {"nsig": nsig}
        if mode == "loop":
            its = np.zeros(nsig, np.int64)

            def call():
                for s in range(nsig):
                    its[s] = d.ctx.bpd_device(B[s], delta, 1.0, x)["iterations"]
            d.ctx.bpd_device(B[0], delta, 1.0, x, maxiter=32)
        else:
            X = torch.zeros((nsig, N), dtype=torch.float64, device="cuda")
            Bt, Xt = B[:nsig].T, X.T  # columns = signals, leading dimensions M and N
            info = {}

            def call():
                info.update(d.ctx.bpd_batch_device(Bt, delta, 1.0, Xt))
            d.ctx.bpd_batch_device(Bt, delta, 1.0, Xt, maxiter=32)  # warm-up: the slots and the group's buffers
        times = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        row["seconds"] = times
        row["signals_per_s"] = [nsig / t for t in times]
        row["iterations"] = (its if mode == "loop" else info["iterations"]).tolist()
        if mode == "batch":  # the batch's results are the loop's
            for s in sorted({0, nsig - 1}):
                one = d.ctx.bpd_device(B[s], delta, 1.0, x)
                assert one["iterations"] == info["iterations"][s] and one["resnorm"] == info["resnorm"][s] and torch.equal(x, X[s]), (nsig, s)
            row["checked_against_csmp_bpd"] = True
        out["rows"].append(row)
    d.close()
    return out


def once(root):
    import torch
    cs, d, B, delta, x = setup(root, 8)
    X = torch.zeros((8, N), dtype=torch.float64, device="cuda")
    d.ctx.bpd_batch_device(B.T, delta, 1.0, X.T, maxiter=64, tol=NEVER)
    for s in range(8):
        d.ctx.bpd_device(B[s], delta, 1.0, x, maxiter=64, tol=NEVER)
    d.close()
    return {"mode": "once", "members": 8, "iterations": 64}


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


KERNELS = ("k_bp_gemm", "k_bp_gemv", "k_sweep_wide", "k_sweep_multi", "k_sweep", "k_bp_update_group", "k_bp_update", "k_ista_axpy_group",
           "k_ista_axpy", "k_ista_resum_group", "k_ista_resum", "k_bpd_pq_group", "k_bpd_pq", "k_bpd_ball_group", "k_bpd_ball", "k_bpd_fold",
           "k_bpd_start", "k_norm2")


def trace(outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, mean_us, total_ms}}"""
    os.makedirs(outdir, exist_ok=True)
    child(["--mode", "once"], limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
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
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("batch", "loop", "once", "ab"), default="batch")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="ab: a built checkout of the parent commit")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nsig", default=",".join(map(str, NSIGS)))
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "bpd_batch_trace"))
    ap.add_argument("--out")
    a = ap.parse_args()
    nsigs = tuple(int(x) for x in a.nsig.split(","))
    if a.mode == "once":
        print(json.dumps(once(a.root)))
        return
    if a.mode != "ab":
        print(json.dumps(measure(a.mode, a.root, a.calls, nsigs)))
        return
    if not a.baseline_root:
        raise SystemExit("--mode ab needs --baseline-root")
    if a.rounds < 2:
        raise SystemExit("--mode ab needs at least two rounds: the spread of each side is part of the result")
    res = {"shape": [M, N, "float32"], "signals": "tools/bench_bpd.py: k = 64 planted atoms, sigma = 1e-2, delta = sigma sqrt(M), rho = 100, tol = 1e-8",
           "baseline": "the parent commit: a loop of csmp_bpd over the same signals", "runs": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    common = ["--calls", str(a.calls), "--nsig", a.nsig]
    for _ in range(a.rounds):  # builds alternated in one session
        res["runs"].append(child(["--mode", "loop", "--root", a.baseline_root] + common, a.limit))
        save()
        res["runs"].append(child(["--mode", "batch", "--root", a.root] + common, a.limit))
        save()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    table = {}
    for nsig in nsigs:
        loop = [x for r in res["runs"] if r["mode"] == "loop" for row in r["rows"] if row["nsig"] == nsig for x in row["signals_per_s"]]
        batch = [x for r in res["runs"] if r["mode"] == "batch" for row in r["rows"] if row["nsig"] == nsig for x in row["signals_per_s"]]
        noise = max(spread(loop), spread(batch))
        ratio = med(batch) / med(loop)
        table[nsig] = {"loop_signals_per_s": med(loop), "loop_spread": spread(loop), "batch_signals_per_s": med(batch), "batch_spread": spread(batch),
                       "ratio": ratio, "faster_beyond_the_spread": ratio - 1.0 > noise, "within_the_spread": abs(ratio - 1.0) <= noise}
    res["table"] = table
    res["condition_met"] = (all(table[n]["faster_beyond_the_spread"] for n in (8, 16) if n in table)
                            and all(table[n]["within_the_spread"] for n in (1,) if n in table))
    save()
    if a.trace:
        res["kernel_trace_of_64_iterations_of_eight_members_and_of_a_loop_of_eight"] = tr = trace(a.trace_dir, a.limit)
        res["step_split_us"] = {k: tr[k]["mean_us"] for k in tr}
        save()
        print(json.dumps(res["step_split_us"]))
    for nsig in nsigs:
        print(nsig, json.dumps(table[nsig]))
    print(json.dumps({"condition_met": res["condition_met"]}))
    if not res["condition_met"]:
        raise SystemExit("the batch is not faster than the parent's loop beyond the spread at nsig = 8 and 16, or nsig = 1 is outside it")


if __name__ == "__main__":
    main()
