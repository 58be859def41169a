"""csmp_somp against the independent solves a caller of the parent commit runs on jointly sparse columns: csmp_omp_batch (up to nsig
supports, nsig appends a step) and csmp_mp_batch (the nearest one-pass-per-step workload), at bench.py's dictionary (4096 x 65536
Float32), k = 256, on planted jointly sparse data: 256 rows shared by all columns, Gaussian coefficients, 5 % noise per column.

    python tools/bench_somp.py --mode somp                       # this tree: csmp_somp, nsig in (8, 16, 64)
    python tools/bench_somp.py --mode baseline [--root D]        # csmp_omp_batch and csmp_mp_batch on the same B (D: another built checkout)
    python tools/bench_somp.py --mode once                       # one solve of 16 columns: for a kernel trace
    python tools/bench_somp.py --mode ab --baseline-root D [--trace] [--out profiles/r24_somp.json]

ab ALTERNATES the two sides in fresh child processes -- `--rounds` times: the baselines on the checkout D (the parent commit, built),
then csmp_somp on this tree --, every child under a time limit of its own, and stops at the first that fails.  A child makes one warm-up
call per nsig and then `--repeats` timed calls by the host clock (every form returns with its results on the host); rounds x repeats
is at least six.  Reported per nsig and side: seconds per call as fastest / median / slowest over all repeats of all rounds, and per
step (a call over the steps it took).  Recorded beside them: the support somp recovered against the planted one, and how many of
omp_batch's supports equal the planted one.  No ratio is fixed in advance.  --trace adds one `rocprofv3 --kernel-trace --stats` run of
`--mode once` in a process of its own: per step the device time of the passes, the pick, the append chain and the projection.
Needs a GPU; there is no fallback, and nothing of the reference tree is read."""
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
K = 256
NOISE = 0.05
SEED = 24_024


def load(root):
    sys.path.insert(0, root)
    from csmp_pkg import load as ld
    return ld()


def problem(nsig):
    """bench.py's dictionary; B = A[:, S] X + noise, |S| = K shared by all columns -> (At, B numpy M x nsig column-major, S sorted)"""
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    import bench
    dev = torch.device("cuda:0")
    At = bench.make_dictionary(torch, dev)
    g = torch.Generator(device=dev).manual_seed(SEED)
    S = torch.randperm(bench.N, generator=g, device=dev)[:K]
    X = torch.randn((K, nsig), generator=g, device=dev, dtype=torch.float64)
    X += torch.sign(X)
    B = At[S].to(torch.float64).T @ X
    E = torch.randn((bench.M, nsig), generator=g, device=dev, dtype=torch.float64)
    B += NOISE * E * (B.norm(dim=0) / E.norm(dim=0))
    torch.cuda.synchronize()
    return At, np.asfortranarray(B.cpu().numpy()), np.sort(S.cpu().numpy())


def measure(mode, root, repeats, nsigs, p):
    import numpy as np
    cs = load(root)
    At, B, S = problem(max(nsigs))
    d = cs.Dictionary(At)
    out = {"mode": mode, "root": os.path.basename(os.path.abspath(root)), "repeats": repeats, "device": d.ctx.device_info()[0],
           "sweep_config": d.ctx.sweep_config(), "rows": []}
    for nsig in nsigs:
        Bn = np.asfortranarray(B[:, :nsig])
        row = {"nsig": nsig}
        forms = {"somp": lambda: d.ctx.somp(Bn, K, 0.0, p)} if mode == "somp" else \
                {"omp_batch": lambda: d.ctx.omp_batch(Bn, K, 0.0), "mp_batch": lambda: d.ctx.mp_batch(Bn, K)}
        for name, call in forms.items():
            res = call()  # warm-up: the slots, the clones' buffers, code objects
            times = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                res = call()
                times.append(time.perf_counter() - t0)
            row[name + "_seconds"] = times
            if name == "somp":
                idx, val, info = res
                row["steps"], row["passes"] = int(info["steps"]), int(info["passes"])
                row["planted_atoms_in_the_support"] = int(np.intersect1d(idx, S).size)
                row["digest"] = [int(idx.sum()), float(val.sum()).hex(), float(info["resnorm"].sum()).hex()]
            elif name == "omp_batch":
                idx, val, nnz = res
                row["omp_batch_supports_equal_to_the_planted_one"] = int(sum(np.array_equal(idx[:nnz[s], s], S) for s in range(nsig)))
                row["omp_batch_distinct_supports"] = len({idx[:nnz[s], s].tobytes() for s in range(nsig)})
        out["rows"].append(row)
    d.close()
    return out


def once(root, p):
    cs = load(root)
    At, B, _ = problem(16)
    d = cs.Dictionary(At)
    warm = d.ctx.somp(B, 2, 0.0, p)[2]  # (code objects, the slot; its launches are in the trace too)
    t0 = time.perf_counter()
    info = d.ctx.somp(B, K, 0.0, p)[2]
    secs = time.perf_counter() - t0
    d.close()
    return {"mode": "once", "nsig": 16, "steps": int(info["steps"]), "passes": int(info["passes"]), "warm_up_steps": int(warm["steps"]),
            "seconds": secs}


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


# a step's parts: the passes (the longer names first), the pick, the append chain, the projection
PARTS = {"pass": ("k_sweep_wide", "k_sweep_multi"), "pick": ("k_somp_pick",), "append": ("k_qr1", "k_qr2", "k_qr3"),
         "project": ("k_somp_project",), "solve": ("k_somp_solve",), "init": ("k_somp_init", "k_init")}


def trace(outdir, limit, p):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> per part {calls, total_ms, us_per_step}"""
    os.makedirs(outdir, exist_ok=True)
    info = child(["--mode", "once", "--p", str(p)], limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
    parts = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            part = next((q for q, names in PARTS.items() if any(n in name for n in names)), None)
            if part:
                e = parts.setdefault(part, {"calls": 0, "total_ms": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    steps = max(info["steps"] + info["warm_up_steps"], 1)  # (every launch of the process is in the trace)
    for e in parts.values():
        e["us_per_step"] = 1e3 * e["total_ms"] / steps
        e["mean_us"] = 1e3 * e["total_ms"] / max(e["calls"], 1)
    in_step = sum(parts[q]["us_per_step"] for q in ("pass", "pick", "append", "project") if q in parts)
    for q in ("pass", "pick", "append", "project"):
        if q in parts:
            parts[q]["share_of_a_step"] = parts[q]["us_per_step"] / in_step
    return {"program": info, "parts": parts, "device_us_per_step": in_step, "wall_us_per_step": 1e6 * info["seconds"] / max(info["steps"], 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("somp", "baseline", "once", "ab"), default="somp")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="ab: a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3, help="ab: how often the two sides take turns")
    ap.add_argument("--repeats", type=int, default=2, help="timed calls per nsig in one child")
    ap.add_argument("--nsig", default=",".join(map(str, NSIGS)))
    ap.add_argument("--p", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "somp_trace"))
    ap.add_argument("--out")
    a = ap.parse_args()
    nsigs = tuple(int(x) for x in a.nsig.split(","))
    if a.mode == "once":
        print(json.dumps(once(a.root, a.p)))
        return
    if a.mode != "ab":
        print(json.dumps(measure(a.mode, a.root, a.repeats, nsigs, a.p)))
        return
    if not a.baseline_root:
        raise SystemExit("--mode ab needs --baseline-root")
    if os.path.abspath(a.baseline_root) == os.path.abspath(a.root):
        raise SystemExit("--baseline-root is the tree under test: the baseline is a built checkout of the parent commit")
    if a.rounds * a.repeats < 6:
        raise SystemExit("rounds x repeats has to be at least six")
    res = {"shape": [4096, 65536, "float32"], "k": K, "p": a.p, "eps": 0.0,
           "signals": f"{K} planted rows shared by all columns, Gaussian coefficients of magnitude >= 1, {NOISE:.0%} noise per column, seed {SEED}",
           "baselines": "a built checkout of the parent commit: csmp_omp_batch and csmp_mp_batch on the same B",
           "schedule": f"{a.rounds} rounds of (baseline child, somp child), {a.repeats} timed calls per nsig and child after a warm-up call",
           "runs": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    common = ["--repeats", str(a.repeats), "--nsig", a.nsig, "--p", str(a.p)]
    for _ in range(a.rounds):
        for mode, root in (("baseline", a.baseline_root), ("somp", a.root)):
            res["runs"].append(child(["--mode", mode, "--root", root] + common, a.limit))
            save()
    med = lambda v: sorted(v)[len(v) // 2]
    table = []
    for nsig in nsigs:
        t = {"nsig": nsig}
        rows = [row for r in res["runs"] for row in r["rows"] if row["nsig"] == nsig]
        somp_rows = [row for row in rows if "somp_seconds" in row]
        t["steps"], t["passes"] = somp_rows[0]["steps"], somp_rows[0]["passes"]
        t["planted_atoms_in_the_support"] = somp_rows[0]["planted_atoms_in_the_support"]
        t["same_bits_in_every_round"] = all(row["digest"] == somp_rows[0]["digest"] for row in somp_rows)
        for name in ("somp", "omp_batch", "mp_batch"):
            v = [s for row in rows for s in row.get(name + "_seconds", [])]
            t[name + "_ms_per_call"] = {"fastest": 1e3 * min(v), "median": 1e3 * med(v), "slowest": 1e3 * max(v), "repeats": len(v)}
        t["somp_us_per_step"] = 1e3 * t["somp_ms_per_call"]["median"] / max(t["steps"], 1)
        t["omp_batch_us_per_step_and_signal"] = 1e3 * t["omp_batch_ms_per_call"]["median"] / (K * nsig)
        t["mp_batch_us_per_step_and_signal"] = 1e3 * t["mp_batch_ms_per_call"]["median"] / (K * nsig)
        base = [row for row in rows if "omp_batch_seconds" in row][0]
        t["omp_batch_supports_equal_to_the_planted_one"] = base["omp_batch_supports_equal_to_the_planted_one"]
        t["omp_batch_distinct_supports"] = base["omp_batch_distinct_supports"]
        t["slowest_somp_beats_the_fastest_omp_batch"] = t["somp_ms_per_call"]["slowest"] < t["omp_batch_ms_per_call"]["fastest"]
        t["slowest_somp_beats_the_fastest_mp_batch"] = t["somp_ms_per_call"]["slowest"] < t["mp_batch_ms_per_call"]["fastest"]
        table.append(t)
    res["table"] = table
    save()
    if a.trace:
        res["kernel_trace_of_sixteen_columns"] = trace(a.trace_dir, a.limit, a.p)
        save()
        print(json.dumps(res["kernel_trace_of_sixteen_columns"]))
    for t in table:
        print(json.dumps(t))


if __name__ == "__main__":
    main()
