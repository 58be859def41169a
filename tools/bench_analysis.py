"""csmp_colnorms / csmp_cumbabel at the benchmark's shape (4096 x 65536 Float32).

    python tools/bench_analysis.py --mode time     # seconds of colnorms, coherence, cumbabel(k = 256) with and without normalize
    python tools/bench_analysis.py --mode torch    # the loop a PyTorch user writes today, Float64 on the card (time yardstick only)
    python tools/bench_analysis.py --mode once     # one cumbabel(k = 256, normalize) and one oblivious start of 128 atoms: the program
                                                   # a kernel trace is taken of (the start runs k_fr_rebuild_lds once on the same shape)
    python tools/bench_analysis.py --mode all [--out profiles/r12_analysis.json]

all runs every step in a fresh child process under a time limit of its own and stops at the first that fails; the kernel trace is one
`rocprofv3 --kernel-trace --stats` run in a process of its own.  It records k_gram_strip's FLOP/s (2 * 128 * N * M per launch), that
rate as a ratio to k_fr_rebuild_lds's in the same run, and the share of the kernel time k_babel_rows takes.  No thresholds.  Needs a
GPU; there is no fallback."""
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
KERNELS = ("k_gram_strip", "k_babel_rows", "k_babel_fold", "k_babel_init", "k_an_root", "k_fr_colnorm2", "k_fr_rebuild_lds")


def make_inputs(n=N):
    """Gaussian atoms of norm about 1 generated on the device, as an (n, M) tensor whose rows are the atoms"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(12)
    At = torch.randn((n, M), generator=g, device="cuda", dtype=torch.float32) / M ** 0.5
    return At.contiguous()


def load():
    sys.path.insert(0, HERE)
    from csmp_pkg import load as ld
    return ld()


def timed(f, calls):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = f()  # (the library's calls return with the work done)
        out.append(time.perf_counter() - t0)
    return out, r


def mode_time(calls, n):
    cs = load()
    d = cs.Dictionary(make_inputs(n))
    out = {"mode": "time", "shape": [M, n, "float32"], "device": d.ctx.device_info()[0], "rows": []}
    d.ctx.cumbabel(1, True)  # warm-up: buffers, code objects
    for name, f in (("colnorms", lambda: d.ctx.colnorms(device=True)),
                    ("coherence", lambda: d.ctx.cumbabel(1, False)),
                    ("coherence_normalize", lambda: d.ctx.cumbabel(1, True)),
                    (f"cumbabel_k{K}", lambda: d.ctx.cumbabel(K, False)),
                    (f"cumbabel_k{K}_normalize", lambda: d.ctx.cumbabel(K, True))):
        secs, r = timed(f, calls)
        row = {"call": name, "seconds": secs, "seconds_median": sorted(secs)[len(secs) // 2]}
        if name != "colnorms":
            row["mu_1"], row["mu_last"], row["pair"] = float(r[0][0]), float(r[0][-1]), list(r[1])
        out["rows"].append(row)
    d.close()
    return out


def mode_torch(calls, n):
    """what a PyTorch-ROCm user writes today: Float64 A[:, blk].T @ A, abs, topk, cumsum, a running maximum over blocks of 128 columns"""
    import torch
    At = make_inputs(n).to(torch.float64)
    out = {"mode": "torch", "shape": [M, n, "float64 copy of the float32 dictionary"], "rows": []}
    for k in (1, K):
        secs = []
        for _ in range(calls + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mu = torch.zeros(k, dtype=torch.float64, device="cuda")
            for q0 in range(0, n, 128):
                G = (At[q0:q0 + 128] @ At.T).abs_()
                rows = torch.arange(G.shape[0], device="cuda")
                G[rows, q0 + rows] = 0.0
                mu = torch.maximum(mu, torch.cumsum(torch.topk(G, k, dim=1).values, dim=1).max(dim=0).values)
            res = mu.cpu()
            secs.append(time.perf_counter() - t0)
        secs = secs[1:]  # (the first is the warm-up)
        out["rows"].append({"call": f"cumbabel_k{k}", "seconds": secs, "seconds_median": sorted(secs)[len(secs) // 2],
                            "mu_1": float(res[0]), "mu_last": float(res[-1])})
    return out


def mode_once(n):
    import numpy as np
    cs = load()
    d = cs.Dictionary(make_inputs(n))
    d.ctx.cumbabel(K, True)
    b = np.random.default_rng(0).standard_normal(M).astype(np.float32)
    d.ctx.srr(b, 128, 1e-12, maxiter=0, initialization=1)  # the oblivious start: one k_fr_rebuild_lds launch of 128 directions
    d.close()
    return {"mode": "once"}


def child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} failed ({p.returncode}): nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def trace(n, outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, total_ns, mean_us}}"""
    os.makedirs(outdir, exist_ok=True)
    child(["--mode", "once", "--n", str(n)], limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
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
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("time", "torch", "once", "all"), default="time")
    ap.add_argument("--n", type=int, default=N, help="columns of the dictionary (default: the benchmark's 65536)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "analysis_trace"), help="where the kernel trace is written")
    a = ap.parse_args()
    if a.mode == "time":
        print(json.dumps(mode_time(a.calls, a.n)))
    elif a.mode == "torch":
        print(json.dumps(mode_torch(a.calls, a.n)))
    elif a.mode == "once":
        print(json.dumps(mode_once(a.n)))
    else:
        res = {"shape": [M, a.n, "float32"], "k": K}
        res["library"] = child(["--mode", "time", "--n", str(a.n), "--calls", str(a.calls)], 420)
        res["measured_on"] = res["library"]["device"]
        res["torch_float64_loop"] = child(["--mode", "torch", "--n", str(a.n), "--calls", "1"], 420)
        kern = res["kernel_trace"] = trace(a.n, a.trace_dir, 300)
        flop = 2.0 * 128 * a.n * M  # per launch of either kernel: 128 directions against every atom
        g, r = kern.get("k_gram_strip"), kern.get("k_fr_rebuild_lds")
        if g:
            res["k_gram_strip_flop_per_s"] = flop / (g["mean_us"] * 1e-6)
        if r:
            res["k_fr_rebuild_lds_flop_per_s"] = flop / (r["mean_us"] * 1e-6)
        if g and r:
            res["k_gram_strip_rate_over_k_fr_rebuild_lds_rate"] = r["mean_us"] / g["mean_us"]
        ours = [kern[k]["total_ns"] for k in KERNELS if k in kern and k != "k_fr_rebuild_lds"]
        if "k_babel_rows" in kern and ours:
            res["k_babel_rows_share_of_kernel_time"] = kern["k_babel_rows"]["total_ns"] / sum(ours)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        for row in res["library"]["rows"] + res["torch_float64_loop"]["rows"]:
            print(row["call"], f'{row["seconds_median"]:.4f} s')
        print(json.dumps({k: v for k, v in res.items() if k.startswith("k_")}))


if __name__ == "__main__":
    main()
