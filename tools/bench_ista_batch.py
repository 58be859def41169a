"""csmp_ista_batch against the caller's loop over csmp_ista, at the benchmark's shape (4096 x 65536 Float32, tools/bench_ista.py's
signals: 256 planted atoms with 5e-3 noise, one support per signal), ISTA and FISTA in the sparse (λ = 1.6) and the dense (λ = 1e-3)
regime.

    python tools/bench_ista_batch.py --mode batch            # this tree: csmp_ista_batch, nsig in (1, 2, 4, 8, 16)
    python tools/bench_ista_batch.py --mode loop [--root D]  # the loop of csmp_ista over the same signals (D: another built checkout)
    python tools/bench_ista_batch.py --mode once --regime sparse   # one batch of eight and a loop of eight, 64 iterations: for a kernel trace
    python tools/bench_ista_batch.py --mode ab --baseline-root D [--rounds 2] [--out profiles/r21_ista_batch.json] [--trace]

ab alternates fresh child processes -- the loop on the baseline checkout D (the parent commit, built), the batch on this tree --, every
child under a time limit of its own, and stops at the first that fails.  Per (regime, method, nsig): signals/s by the host clock around
the call (device pointers in and out; both forms return with the work done).  In every batch child columns 0 and nsig - 1 are compared
with csmp_ista's bits, and ab compares the resnorms of the parent's loop with the batch's, all of them, bit for bit.  Reported: the
median of each side, their ratio, and each side's spread between all its readings ((max - min) / median).  The condition: in the
sparse regime at nsig = 8 and 16 the batch beats the loop by more than the larger of the two spreads; everything else is recorded
without a threshold.  --trace adds one `rocprofv3 --kernel-trace --stats` run of `--mode once` per regime, each in a process of its own.
Needs a GPU; there is no fallback."""
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
from bench_ista import K, M, N, REGIMES, load, make_inputs  # noqa: E402
NSIGS = (1, 2, 4, 8, 16)


def make_signals(nsig):
    """bench_ista.py's dictionary, step size and signal (row 0); rows 1 .. nsig - 1 are made by the same recipe on supports of their own"""
    import torch
    A32, b, alpha = make_inputs()
    B = torch.empty((nsig, M), dtype=torch.float32, device="cuda")
    B[0] = b
    for s in range(1, nsig):
        g = torch.Generator(device="cuda").manual_seed(1100 + s)
        S = torch.randperm(N, generator=g, device="cuda")[:K]
        v = torch.where(torch.rand(K, generator=g, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
        B[s] = (v @ A32[S].to(torch.float64) + 5e-3 * torch.randn(M, generator=g, device="cuda", dtype=torch.float64)).to(torch.float32)
    return A32, B, alpha


def measure(mode, root, iters, calls, nsigs, regimes):
    import torch
    cs = load(root)
    A32, B, alpha = make_signals(max(nsigs))
    d = cs.Dictionary(A32)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    out = {"mode": mode, "root": os.path.basename(os.path.abspath(root)), "iters": iters, "calls": calls, "stepsize": alpha,
           "device": d.ctx.device_info()[0], "rows": []}
    if mode == "batch":
        out["sweep_config"] = d.ctx.sweep_config()
    for regime in regimes:
        lam = REGIMES[regime]
        for accel in (False, True):
            kw = dict(maxiter=iters, stepsize=alpha, accel=accel)
            d.ctx.ista_device(B[0], lam, x, maxiter=8, stepsize=alpha, accel=accel)  # warm-up: buffers, code objects
            for nsig in nsigs:
                row = {"regime": regime, "lambda": lam, "method": "fista" if accel else "ista", "nsig": nsig}
                rn = [0.0] * nsig
                if mode == "loop":
                    def call():
                        for s in range(nsig):
                            rn[s] = d.ctx.ista_device(B[s], lam, x, **kw)
                else:
                    X = torch.zeros((nsig, N), dtype=torch.float64, device="cuda")
                    Bt, Xt = B[:nsig].T, X.T  # columns = signals, leading dimensions M and N

                    def call():
                        rn[:] = d.ctx.ista_batch_device(Bt, lam, Xt, **kw).tolist()
                    d.ctx.ista_batch_device(Bt, lam, Xt, maxiter=4, stepsize=alpha, accel=accel)  # warm-up: the slots and the group's buffers
                times = []
                for _ in range(calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    times.append(time.perf_counter() - t0)
                row["seconds"] = times
                row["signals_per_s"] = [nsig / t for t in times]
                row["us_per_signal_iteration"] = [1e6 * t / (nsig * iters) for t in times]
                row["resnorm_hex"] = [float(v).hex() for v in rn]
                if mode == "batch":  # the batch's results are csmp_ista's
                    row["nnz_of_results"] = torch.count_nonzero(X, dim=1).tolist()
                    for s in sorted({0, nsig - 1}):
                        one = d.ctx.ista_device(B[s], lam, x, **kw)
                        assert one == rn[s] and torch.equal(x, X[s]), (regime, accel, nsig, s)
                    row["checked_against_csmp_ista"] = True
                out["rows"].append(row)
    d.close()
    return out


def once(root, regime, iters):
    import torch
    cs = load(root)
    A32, B, alpha = make_signals(8)
    d = cs.Dictionary(A32)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    X = torch.zeros((8, N), dtype=torch.float64, device="cuda")
    d.ctx.ista_batch_device(B.T, REGIMES[regime], X.T, maxiter=iters, stepsize=alpha)
    for s in range(8):
        d.ctx.ista_device(B[s], REGIMES[regime], x, maxiter=iters, stepsize=alpha)
    nnz = torch.count_nonzero(X, dim=1).tolist()
    d.close()
    return {"mode": "once", "regime": regime, "members": 8, "iterations": iters, "nnz_of_results": nnz}


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


KERNELS = ("k_sweep_wide", "k_sweep_multi", "k_sweep", "k_ista_update_group", "k_ista_update", "k_ista_axpy_group", "k_ista_axpy",
           "k_ista_resum_group", "k_ista_resum", "k_norm2", "k_init")


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
    return {"program": info, "kernels": kernels}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("batch", "loop", "once", "ab"), default="batch")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="ab: a built checkout of the parent commit")
    ap.add_argument("--regime", choices=tuple(REGIMES) + ("both",), default="both")
    ap.add_argument("--iters", type=int, default=192, help="iterations of every solve (once: 64)")
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nsig", default=",".join(map(str, NSIGS)))
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "ista_batch_trace"))
    ap.add_argument("--out")
    a = ap.parse_args()
    nsigs = tuple(int(x) for x in a.nsig.split(","))
    regimes = tuple(REGIMES) if a.regime == "both" else (a.regime,)
    if a.mode == "once":
        print(json.dumps(once(a.root, regimes[0], 64)))
        return
    if a.mode != "ab":
        print(json.dumps(measure(a.mode, a.root, a.iters, a.calls, nsigs, regimes)))
        return
    if not a.baseline_root:
        raise SystemExit("--mode ab needs --baseline-root")
    if a.rounds < 2:
        raise SystemExit("--mode ab needs at least two rounds: the spread of each side is part of the result")
    res = {"shape": [M, N, "float32"], "signals": "tools/bench_ista.py: 256 planted atoms, 5e-3 noise, one support per signal", "regimes": REGIMES,
           "iters": a.iters, "baseline": "the parent commit: a loop of csmp_ista over the same signals", "runs": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    common = ["--iters", str(a.iters), "--calls", str(a.calls), "--nsig", a.nsig, "--regime", a.regime]
    for _ in range(a.rounds):  # builds alternated in one session
        res["runs"].append(child(["--mode", "loop", "--root", a.baseline_root] + common, a.limit))
        save()
        res["runs"].append(child(["--mode", "batch", "--root", a.root] + common, a.limit))
        save()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    table, same_bits = [], True
    for regime in regimes:
        for method in ("ista", "fista"):
            for nsig in nsigs:
                rows = {m: [row for r in res["runs"] if r["mode"] == m for row in r["rows"]
                            if (row["regime"], row["method"], row["nsig"]) == (regime, method, nsig)] for m in ("loop", "batch")}
                loop = [x for row in rows["loop"] for x in row["signals_per_s"]]
                batch = [x for row in rows["batch"] for x in row["signals_per_s"]]
                same_bits = same_bits and len({tuple(row["resnorm_hex"]) for m in rows for row in rows[m]}) == 1
                noise = max(spread(loop), spread(batch))
                table.append({"regime": regime, "method": method, "nsig": nsig, "loop_signals_per_s": med(loop), "loop_spread": spread(loop),
                              "batch_signals_per_s": med(batch), "batch_spread": spread(batch), "ratio": med(batch) / med(loop),
                              "loop_us_per_signal_iteration": 1e6 / (med(loop) * a.iters), "batch_us_per_signal_iteration": 1e6 / (med(batch) * a.iters),
                              "faster_beyond_the_spread": med(batch) / med(loop) - 1.0 > noise})
    res["table"] = table
    res["resnorms_of_the_parents_loop_and_the_batch_agree_bit_for_bit"] = same_bits
    res["condition_met"] = same_bits and all(t["faster_beyond_the_spread"] for t in table if t["regime"] == "sparse" and t["nsig"] in (8, 16))
    save()
    if a.trace:
        res["kernel_trace_of_64_iterations_of_eight_members_and_of_a_loop_of_eight"] = {r: trace(r, os.path.join(a.trace_dir, r), a.limit) for r in regimes}
        save()
        for r, t in res["kernel_trace_of_64_iterations_of_eight_members_and_of_a_loop_of_eight"].items():
            print(r, json.dumps({k: round(v["mean_us"], 2) for k, v in t["kernels"].items()}))
    for t in table:
        print(json.dumps(t))
    print(json.dumps({"condition_met": res["condition_met"], "same_bits": same_bits}))
    if not res["condition_met"]:
        raise SystemExit("the batch is not faster than the parent's loop beyond the spread in the sparse regime at nsig = 8 and 16")


if __name__ == "__main__":
    main()
