"""csmp_ompr_batch against the two ways a caller had to run ompr for many signals, at bench.py --workload ompr's construction: the
configs[1] dictionary (4096 x 65536 Float32), k = 256, signals with 8 planted atoms more than k and noise 0.3, delta = 1e-6.

    python tools/bench_ompr_batch.py --mode batch                   # this tree: csmp_ompr_batch, nsig in (8, 16, 64)
    python tools/bench_ompr_batch.py --mode loop [--root D]         # the loop of csmp_ompr over the same signals (D: another built checkout)
    python tools/bench_ompr_batch.py --mode inflight [--root D]     # solve_in_flight(..., in_flight=3) over the same signals
    python tools/bench_ompr_batch.py --mode once                    # one batch of eight: for a kernel trace
    python tools/bench_ompr_batch.py --mode ab --baseline-root D [--trace] [--out profiles/r23_ompr_batch.json]

ab runs fresh child processes in turn -- the loop and the three solves in flight on the baseline checkout D (the parent commit, built),
the batch on this tree --, every child under a time limit of its own, and stops at the first that fails.  Per nsig: a warm-up call, then
`--repeats` timed calls by the host clock (every form returns with the results on the host); solves/s as min / median / max.  The batch
child compares every column with csmp_ompr's bits, and ab compares the iterations and a digest of every result of the parent's loop with
the batch's.  Acceptance: at every nsig the batch's slowest repeat is faster than the fastest repeat of both baselines.  Also recorded:
the share of signals solved alone, and the acquisition's time per member (a batch with maxiter = 0 is the starts, their passes and the
acquisitions).  --trace adds one `rocprofv3 --kernel-trace --stats` run of `--mode once` in a process of its own: the launches and the
device time of a tick.  Needs a GPU; there is no fallback, and nothing of the reference tree is read."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSIGS = (8, 16, 64)
DELTA = 1e-6


def load(root):
    sys.path.insert(0, root)
    from csmp_pkg import load as ld
    return ld()


def problem(nsig):
    """bench.py's dictionary and run_twostage's signals (signal s: seed 31337 + s), as numpy columns"""
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    import bench
    dev = torch.device("cuda:0")
    At = bench.make_dictionary(torch, dev)
    M, N, K = bench.M, bench.N, bench.K_ATOMS
    cols = []
    for s in range(nsig):
        g = torch.Generator(device=dev).manual_seed(31_337 + s)
        idx = torch.randperm(N, generator=g, device=dev)[:K + 8]
        sign = torch.randint(0, 2, (K + 8,), generator=g, device=dev).to(torch.float64) * 2 - 1
        e = torch.randn(M, generator=g, device=dev, dtype=torch.float64)
        cols.append(((At[idx].to(torch.float64) * sign[:, None]).sum(0) + e * (0.3 / e.norm())).cpu().numpy())
    torch.cuda.synchronize()
    return At, np.asfortranarray(np.stack(cols, axis=1)), K


def digest(idx, val):
    return [int(idx.sum()), float(val.sum()).hex(), int(len(idx))]


def measure(mode, root, repeats, nsigs):
    import numpy as np
    cs = load(root)
    At, B, K = problem(max(nsigs))
    d = cs.Dictionary(At)
    out = {"mode": mode, "root": os.path.basename(os.path.abspath(root)), "repeats": repeats, "device": d.ctx.device_info()[0], "rows": []}
    if mode == "batch":
        out["sweep_config"] = d.ctx.sweep_config()
    sigs = [np.ascontiguousarray(B[:, s]) for s in range(B.shape[1])]
    one = lambda c, b: c.ompr(b, K, DELTA)
    for nsig in nsigs:
        row = {"nsig": nsig}
        res = [None] * nsig
        if mode == "loop":
            def call():
                res[:] = [one(d.ctx, sigs[s]) for s in range(nsig)]
        elif mode == "inflight":
            def call():
                res[:] = cs.solve_in_flight(d, sigs[:nsig], one, in_flight=3)
        else:
            Bn = np.asfortranarray(B[:, :nsig])
            info = {}

            def call():
                idx, val, nnz, inf = d.ctx.ompr_batch(Bn, K, DELTA)
                res[:] = [(idx[:nnz[s], s], val[:nnz[s], s], int(inf["iterations"][s])) for s in range(nsig)]
                info.update(inf)
        call()  # warm-up: the slots, the clones' buffers, code objects
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        if mode == "batch":
            alone = np.asarray(info["solved_alone"])
            row["solved_alone"] = int(alone.sum())
            for s in range(nsig):  # the batch's results are csmp_ompr's
                r = one(d.ctx, sigs[s])
                assert np.array_equal(r[0], res[s][0]) and np.array_equal(r[1], res[s][1]) and r[2] == res[s][2], (nsig, s)
            row["checked_against_csmp_ompr"] = True
            t0 = time.perf_counter()
            d.ctx.ompr_batch(Bn, K, DELTA, 0)  # the starts, their passes and the acquisitions alone
            row["acquisition_ms_per_member"] = 1e3 * (time.perf_counter() - t0) / nsig
        row["seconds"] = times
        row["solves_per_s"] = [nsig / t for t in times]
        row["iterations"] = [int(r[2]) for r in res]
        row["digest"] = [digest(r[0], r[1]) for r in res]
        out["rows"].append(row)
    d.close()
    return out


def once(root):
    import numpy as np
    cs = load(root)
    At, B, K = problem(8)
    d = cs.Dictionary(At)
    d.ctx.ompr_batch(B, K, DELTA, 1)
    t0 = time.perf_counter()
    info = d.ctx.ompr_batch(B, K, DELTA)[3]
    secs = time.perf_counter() - t0
    d.close()
    return {"mode": "once", "members": 8, "iterations": np.asarray(info["iterations"]).tolist(), "batch_seconds": secs}


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


KERNELS = ("k_sweep_wide", "k_sweep_multi", "k_sweep_short", "k_sweep", "k_ompr_pick_group", "k_ompr_pick", "k_swap_dots_group", "k_swap_dots",
           "k_swap_ufin_group", "k_swap_ufin", "k_swap_commit_res_group", "k_swap_commit_res", "k_swap_rsum_group", "k_swap_rsum",
           "k_swap_land_group", "k_swap_init", "k_land_multi", "k_init", "k_tinv_build", "k_rs_", "k_top_")
TICK = ("k_sweep_wide", "k_sweep_multi", "k_ompr_pick_group", "k_swap_dots_group", "k_swap_ufin_group", "k_swap_commit_res_group",
        "k_swap_rsum_group", "k_swap_land_group")


def trace(outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, mean_us, total_ms}}"""
    os.makedirs(outdir, exist_ok=True)
    info = child(["--mode", "once"], limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
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
    ticks = kernels.get("k_ompr_pick_group", {}).get("calls", 0)
    return {"program": info, "kernels": kernels, "ticks_with_running_members_warm_up_included": ticks,
            "launches_per_tick": len(TICK) - 1,  # (one of the two passes)
            "device_us_per_tick": 1e3 * sum(kernels[k]["total_ms"] for k in TICK if k in kernels) / max(ticks, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("batch", "loop", "inflight", "once", "ab"), default="batch")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="ab: a built checkout of the parent commit")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nsig", default=",".join(map(str, NSIGS)))
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "ompr_batch_trace"))
    ap.add_argument("--out")
    a = ap.parse_args()
    nsigs = tuple(int(x) for x in a.nsig.split(","))
    if a.mode == "once":
        print(json.dumps(once(a.root)))
        return
    if a.mode != "ab":
        print(json.dumps(measure(a.mode, a.root, a.repeats, nsigs)))
        return
    if not a.baseline_root:
        raise SystemExit("--mode ab needs --baseline-root")
    if os.path.abspath(a.baseline_root) == os.path.abspath(a.root):
        raise SystemExit("--baseline-root is the tree under test: the baseline is a built checkout of the parent commit")
    res = {"shape": [4096, 65536, "float32"], "k": 256, "delta": DELTA,
           "signals": "bench.py --workload ompr's: 264 planted atoms, noise 0.3, seed 31337 + s",
           "baselines": "a built checkout of the parent commit: the loop over csmp_ompr, and solve_in_flight(..., in_flight=3)", "runs": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    common = ["--repeats", str(a.repeats), "--nsig", a.nsig]
    for mode, root in (("loop", a.baseline_root), ("inflight", a.baseline_root), ("batch", a.root)):
        res["runs"].append(child(["--mode", mode, "--root", root] + common, a.limit))
        save()
    med = lambda v: sorted(v)[len(v) // 2]
    by = {r["mode"]: {row["nsig"]: row for row in r["rows"]} for r in res["runs"]}
    table, same_bits = [], True
    for nsig in nsigs:
        rows = {m: by[m][nsig] for m in ("loop", "inflight", "batch")}
        same_bits = same_bits and json.dumps([rows["loop"]["iterations"], rows["loop"]["digest"]]) == json.dumps([rows["batch"]["iterations"], rows["batch"]["digest"]])
        t = {"nsig": nsig}
        for m in rows:
            v = rows[m]["solves_per_s"]
            t[m + "_solves_per_s"] = {"min": min(v), "median": med(v), "max": max(v)}
        t["batch_over_loop"] = t["batch_solves_per_s"]["median"] / t["loop_solves_per_s"]["median"]
        t["batch_over_inflight"] = t["batch_solves_per_s"]["median"] / t["inflight_solves_per_s"]["median"]
        t["solved_alone_share"] = rows["batch"]["solved_alone"] / nsig
        t["acquisition_ms_per_member"] = rows["batch"]["acquisition_ms_per_member"]
        t["iterations_per_solve"] = sum(rows["batch"]["iterations"]) / nsig
        t["slowest_batch_beats_the_fastest_of_both_baselines"] = t["batch_solves_per_s"]["min"] > max(t["loop_solves_per_s"]["max"],
                                                                                                      t["inflight_solves_per_s"]["max"])
        table.append(t)
    res["table"] = table
    res["results_of_the_parents_loop_and_the_batch_agree_bit_for_bit"] = same_bits
    res["condition_met"] = same_bits and all(t["slowest_batch_beats_the_fastest_of_both_baselines"] for t in table if t["nsig"] >= 8)
    save()
    if a.trace:
        res["kernel_trace_of_a_batch_of_eight"] = trace(a.trace_dir, a.limit)
        save()
        t = res["kernel_trace_of_a_batch_of_eight"]
        print(json.dumps({k: round(v["mean_us"], 2) for k, v in t["kernels"].items()}), "us per tick", round(t["device_us_per_tick"], 1))
    for t in table:
        print(json.dumps(t))
    print(json.dumps({"condition_met": res["condition_met"], "same_bits": same_bits}))
    if not res["condition_met"]:
        raise SystemExit("the batch's slowest repeat does not beat the fastest repeat of both baselines, or the bits differ")


if __name__ == "__main__":
    main()
