"""csmp_fsbl_batch against the caller's loop over csmp_fsbl, at 4096 x 65536 Float32, 1024 x 65536 Float32 and 2048 x 32768 Float64
(tools/bench_fsbl.py's data: 64 planted atoms, sigma = 1e-2, noise of norm sigma / 2, one support per signal), every solve run to
convergence.

    python tools/bench_fsbl_batch.py --mode batch --shape f32        # this tree: csmp_fsbl_batch, nsig in (2, 4, 8, 16)
    python tools/bench_fsbl_batch.py --mode loop --shape f32 [--root D]   # the loop of csmp_fsbl over the same signals (D: another built checkout)
    python tools/bench_fsbl_batch.py --mode once --shape f32         # one batch of eight and a loop of eight: for a kernel trace
    python tools/bench_fsbl_batch.py --mode ab --baseline-root D [--rounds 2] [--out profiles/r22_fsbl_batch.json] [--trace]

ab alternates fresh child processes -- the loop on the baseline checkout D (the parent commit, built), the batch on this tree --, every
child under a time limit of its own, and stops at the first that fails.  Per (shape, nsig): signals/s by the host clock around the call
(device pointers in and out; both forms return with the work done).  In every batch child columns 0 and nsig - 1 are compared with
csmp_fsbl's bits, and ab compares the iterations and a digest of every x of the parent's loop with the batch's, bit for bit.  Reported:
the median of each side, their ratio, and each side's spread between all its readings ((max - min) / median).  No speed-up is asked for;
the condition is that at nsig = 8 the batch is not slower than the parent's loop beyond the larger of the two spreads, on every shape.
--trace adds one `rocprofv3 --kernel-trace --stats` run of `--mode once` per shape, each in a process of its own: the kernels' shares,
the ticks (launches of k_fsbl_score_group) and the time per tick.  Needs a GPU; there is no fallback."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"f32": (4096, 65536, "float32"), "flat": (1024, 65536, "float32"), "f64": (2048, 32768, "float64")}
NSIGS = (2, 4, 8, 16)
SIGMA = 1e-2
K = 64
MAXITER = 1000


def load(root):
    sys.path.insert(0, root)
    from csmp_pkg import load as ld
    return ld()


def make_signals(M, N, dtype, nsig):
    """tools/bench_fsbl.py's dictionary; row s of B: a planted +-1 signal on K atoms of its own, plus noise of norm sigma / 2"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(17)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float32)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(getattr(torch, dtype)).contiguous()
    B = torch.empty((nsig, M), dtype=torch.float64, device="cuda")
    for s in range(nsig):
        gs = torch.Generator(device="cuda").manual_seed(1700 + s)
        S = torch.sort(torch.randperm(N, generator=gs, device="cuda")[:K]).values
        v = torch.where(torch.rand(K, generator=gs, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
        e = torch.randn(M, generator=gs, device="cuda", dtype=torch.float64)
        B[s] = v @ At[S].to(torch.float64) + e * (SIGMA / 2 / float(e.norm()))
    return At, B


def digest(x):
    return [float(x.sum()).hex(), float(x.abs().max()).hex(), int((x != 0).sum())]


def measure(mode, root, shape, calls, nsigs):
    import torch
    cs = load(root)
    M, N, dtype = SHAPES[shape]
    At, B = make_signals(M, N, dtype, max(nsigs))
    d = cs.Dictionary(At)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    Xall = torch.zeros((max(nsigs), N), dtype=torch.float64, device="cuda")  # row s: the result of signal s, whichever form wrote it
    out = {"mode": mode, "root": os.path.basename(os.path.abspath(root)), "shape": shape, "calls": calls, "device": d.ctx.device_info()[0], "rows": []}
    if mode == "batch":
        out["sweep_config"] = d.ctx.sweep_config()
    d.ctx.fsbl_device(B[0], SIGMA ** 2, x, maxiter=2)  # warm-up: buffers, code objects
    for nsig in nsigs:
        row = {"nsig": nsig}
        its = [0] * nsig
        X = Xall[:nsig]
        if mode == "loop":
            def call():
                for s in range(nsig):
                    its[s] = d.ctx.fsbl_device(B[s], SIGMA ** 2, X[s], maxiter=MAXITER)["iterations"]
        else:
            Bt, Xt = B[:nsig].T, X.T  # columns = signals, leading dimensions M and N

            def call():
                its[:] = d.ctx.fsbl_batch_device(Bt, SIGMA ** 2, Xt, maxiter=MAXITER)["iterations"].tolist()
            d.ctx.fsbl_batch_device(Bt, SIGMA ** 2, Xt, maxiter=2)  # warm-up: the slots and the members' buffers
        times = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        dig = [digest(X[s]) for s in range(nsig)]  # (outside the timed calls, for both forms)
        if mode == "batch":  # the batch's results are csmp_fsbl's
            for s in sorted({0, nsig - 1}):
                one = d.ctx.fsbl_device(B[s], SIGMA ** 2, x, maxiter=MAXITER)
                assert one["iterations"] == its[s] and torch.equal(x, X[s]), (shape, nsig, s)
            row["checked_against_csmp_fsbl"] = True
        row["seconds"] = times
        row["signals_per_s"] = [nsig / t for t in times]
        row["iterations"] = [int(i) for i in its]
        row["us_per_signal_pass"] = [1e6 * t / sum(its) for t in times]
        row["digest"] = dig
        out["rows"].append(row)
    d.close()
    return out


def once(root, shape):
    import torch
    cs = load(root)
    M, N, dtype = SHAPES[shape]
    At, B = make_signals(M, N, dtype, 8)
    d = cs.Dictionary(At)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    X = torch.zeros((8, N), dtype=torch.float64, device="cuda")
    d.ctx.fsbl_batch_device(B.T, SIGMA ** 2, X.T, maxiter=2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = d.ctx.fsbl_batch_device(B.T, SIGMA ** 2, X.T, maxiter=MAXITER)
    secs = time.perf_counter() - t0
    for s in range(8):
        d.ctx.fsbl_device(B[s], SIGMA ** 2, x, maxiter=MAXITER)
    d.close()
    return {"mode": "once", "shape": shape, "members": 8, "iterations": info["iterations"].tolist(), "batch_seconds": secs}


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


KERNELS = ("k_sweep_wide", "k_sweep_multi", "k_sweep_short", "k_sweep", "k_fsbl_score_group", "k_fsbl_score", "k_fsbl_pick_group", "k_fsbl_pick",
           "k_fsbl_col_group", "k_fsbl_col", "k_fsbl_gemv_group", "k_bp_gemv", "k_fsbl_rank1_group", "k_fsbl_rank1", "k_fsbl_eye",
           "k_fr_colnorm2", "k_land_multi", "k_init")


def trace(shape, outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, mean_us, total_ms}}"""
    os.makedirs(outdir, exist_ok=True)
    info = child(["--mode", "once", "--shape", shape], limit,
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
    ticks = kernels.get("k_fsbl_score_group", {}).get("calls", 0)
    group = [k for k in kernels if k.endswith("_group") or k in ("k_sweep_wide", "k_sweep_multi")]
    return {"program": info, "kernels": kernels, "ticks_with_the_warm_up": ticks,
            "device_us_per_tick": 1e3 * sum(kernels[k]["total_ms"] for k in group) / max(ticks, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("batch", "loop", "once", "ab"), default="batch")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="ab: a built checkout of the parent commit")
    ap.add_argument("--shape", choices=tuple(SHAPES) + ("all",), default="all")
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nsig", default=",".join(map(str, NSIGS)))
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "fsbl_batch_trace"))
    ap.add_argument("--out")
    a = ap.parse_args()
    nsigs = tuple(int(x) for x in a.nsig.split(","))
    shapes = tuple(SHAPES) if a.shape == "all" else (a.shape,)
    if a.mode == "once":
        print(json.dumps(once(a.root, shapes[0])))
        return
    if a.mode != "ab":
        for shape in shapes:
            print(json.dumps(measure(a.mode, a.root, shape, a.calls, nsigs)))
        return
    if not a.baseline_root:
        raise SystemExit("--mode ab needs --baseline-root")
    if a.rounds < 2:
        raise SystemExit("--mode ab needs at least two rounds: the spread of each side is part of the result")
    res = {"shapes": SHAPES, "signals": "tools/bench_fsbl.py's data: 64 planted atoms, sigma 1e-2, noise of norm sigma / 2, one support per signal",
           "maxiter": MAXITER, "baseline": "the parent commit: a loop of csmp_fsbl over the same signals",
           "traffic_model_arithmetic_not_measured": {"f32": "8 x (1 GiB + 384 MiB) against 1 GiB + 8 x 384 MiB a step: 2.7 in bytes",
                                                     "flat": "8 x (256 MiB + 24 MiB) against 256 MiB + 8 x 24 MiB: 5.0 in bytes",
                                                     "f64": "8 x (512 MiB + 96 MiB) against 512 MiB + 8 x 96 MiB: 3.8 in bytes"}, "runs": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    for shape in shapes:
        common = ["--calls", str(a.calls), "--nsig", a.nsig, "--shape", shape]
        for _ in range(a.rounds):  # builds alternated in one session
            res["runs"].append(child(["--mode", "loop", "--root", a.baseline_root] + common, a.limit))
            save()
            res["runs"].append(child(["--mode", "batch", "--root", a.root] + common, a.limit))
            save()
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    table, same_bits = [], True
    for shape in shapes:
        for nsig in nsigs:
            rows = {m: [row for r in res["runs"] if r["mode"] == m and r["shape"] == shape for row in r["rows"] if row["nsig"] == nsig]
                    for m in ("loop", "batch")}
            loop = [x for row in rows["loop"] for x in row["signals_per_s"]]
            batch = [x for row in rows["batch"] for x in row["signals_per_s"]]
            same_bits = same_bits and len({json.dumps([row["iterations"], row["digest"]]) for m in rows for row in rows[m]}) == 1
            noise = max(spread(loop), spread(batch))
            passes = sum(rows["loop"][0]["iterations"])
            table.append({"shape": shape, "nsig": nsig, "passes": passes, "loop_signals_per_s": med(loop), "loop_spread": spread(loop),
                          "batch_signals_per_s": med(batch), "batch_spread": spread(batch), "ratio": med(batch) / med(loop),
                          "loop_us_per_signal_pass": 1e6 * nsig / (med(loop) * passes), "batch_us_per_signal_pass": 1e6 * nsig / (med(batch) * passes),
                          "not_slower_beyond_the_spread": med(batch) / med(loop) >= 1.0 - noise})
    res["table"] = table
    res["results_of_the_parents_loop_and_the_batch_agree_bit_for_bit"] = same_bits
    res["condition_met"] = same_bits and all(t["not_slower_beyond_the_spread"] for t in table if t["nsig"] == 8)
    save()
    if a.trace:
        res["kernel_trace_of_a_batch_of_eight_and_of_a_loop_of_eight"] = {s: trace(s, os.path.join(a.trace_dir, s), a.limit) for s in shapes}
        save()
        for s, t in res["kernel_trace_of_a_batch_of_eight_and_of_a_loop_of_eight"].items():
            print(s, json.dumps({k: round(v["mean_us"], 2) for k, v in t["kernels"].items()}), "us per tick", round(t["device_us_per_tick"], 1))
    for t in table:
        print(json.dumps(t))
    print(json.dumps({"condition_met": res["condition_met"], "same_bits": same_bits}))
    if not res["condition_met"]:
        raise SystemExit("the batch at eight signals is slower than the parent's loop beyond the spread, or the bits differ")


if __name__ == "__main__":
    main()
