"""csmp_ard_weights / csmp_ista_reweighted at the benchmark's shape (4096 x 65536 Float32), supports of k = 256 and k = 1024 atoms.

    python tools/bench_reweight.py --mode weights --k 256   # seconds of ard_weights at iter = 1 and iter = 8; the N-pass alone, fused
                                                            # (k_ard_forms) and split (k_fr_rebuild_lds per 128 directions + a root)
    python tools/bench_reweight.py --mode torch --k 256     # the Woodbury form a PyTorch user writes, Float64 on the card, and the
                                                            # library's weights against it
    python tools/bench_reweight.py --mode solve             # ista_ard, 8 outer solves of 256 iterations, against 8 plain ista calls
    python tools/bench_reweight.py --mode once --k 256      # one ard_weights (iter = 1) and one oblivious start of 128 atoms: the
                                                            # program a kernel trace is taken of
    python tools/bench_reweight.py --mode all [--out profiles/r14_reweight.json]

all runs every step in a fresh child process under a time limit of its own and stops at the first that fails; the kernel trace is one
`rocprofv3 --kernel-trace --stats` run in a process of its own.  It records the time of k_ard_forms per 128 directions and its FLOP/s
(2 * 128 * N * M per block) beside k_fr_rebuild_lds's in the same run.  No thresholds.  Needs a GPU; there is no fallback."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N = 4096, 65536
EPS = 1e-2
KERNELS = ("k_ard_forms", "k_rw_dirs", "k_rw_support", "k_rw_assemble", "k_rw_gram_sym", "k_rw_inner_w", "k_gather_cols", "k_gram", "k_chol_row",
           "k_chol_step", "k_wgemm", "k_fr_rebuild_lds")


def make_inputs(k, n=N):
    """Gaussian atoms of norm about 1 generated on the device ((n, M): rows are atoms), an x with k entries of size 0.5 .. 1.5, weights in
    [0.5, 2]"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(14)
    At = (torch.randn((n, M), generator=g, device="cuda", dtype=torch.float32) / M ** 0.5).contiguous()
    S = torch.randperm(n, generator=g, device="cuda")[:k]
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    x[S] = (0.5 + torch.rand(k, generator=g, device="cuda", dtype=torch.float64)) * torch.where(torch.rand(k, generator=g, device="cuda") < 0.5, -1.0, 1.0)
    w = 0.5 + 1.5 * torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    return At, x, w


def load():
    sys.path.insert(0, HERE)
    from csmp_pkg import load as ld
    return ld()


def timed(f, calls):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()  # (the library's calls return with the work done)
        out.append(time.perf_counter() - t0)
    return out


def med(v):
    return sorted(v)[len(v) // 2]


def mode_weights(k, calls):
    import torch
    cs = load()
    At, x, w = make_inputs(k)
    d = cs.Dictionary(At)
    out = torch.empty_like(w)
    res = {"mode": "weights", "shape": [M, N, "float32"], "k": k, "device": d.ctx.device_info()[0]}
    d.ctx.ard_weights_device(x, w, out, EPS, 1)  # warm-up: buffers, code objects
    for it in (1, 8):
        secs = timed(lambda: d.ctx.ard_weights_device(x, w, out, EPS, it), calls)
        res[f"ard_weights_iter{it}_seconds"] = secs
        res[f"ard_weights_iter{it}_seconds_median"] = med(secs)
    blocks = (k + 127) // 128
    for variant, name in ((0, "fused_k_ard_forms"), (1, "split_k_fr_rebuild_lds")):
        ms, diff = d.ctx.bench_ard_forms(variant, 5, EPS)
        res[name + "_ms"] = ms
        res[name + "_ms_per_128_directions"] = ms / blocks
        res[name + "_flop_per_s"] = 2.0 * 128 * blocks * N * M / (ms * 1e-3)
        res["fused_against_split_max_abs_diff"] = diff
    d.close()
    return res


def woodbury(At64, x, w, it):
    """K = eps I + A_S diag(d_S) A_S' (M x M), Cholesky, a_j' K^-1 a_j for every atom in blocks of 8192"""
    import torch
    S = torch.nonzero(x).flatten()
    for _ in range(it):
        AS = At64[S]  # (k, M)
        d = x[S].abs() / w[S]
        K = EPS * torch.eye(M, dtype=torch.float64, device="cuda") + AS.T @ (AS * d[:, None])
        L = torch.linalg.cholesky(K)
        q = torch.empty(At64.shape[0], dtype=torch.float64, device="cuda")
        for j0 in range(0, At64.shape[0], 8192):
            Y = torch.linalg.solve_triangular(L, At64[j0:j0 + 8192].T, upper=False)
            q[j0:j0 + 8192] = (Y * Y).sum(dim=0)
        w = torch.sqrt(torch.clamp(q, min=0.0))
    return w


def mode_torch(k, calls):
    import torch
    cs = load()
    At, x, w = make_inputs(k)
    d = cs.Dictionary(At)
    At64 = At.to(torch.float64)
    res = {"mode": "torch", "k": k}
    for it in (1, 8):
        got = torch.empty_like(w)
        d.ctx.ard_weights_device(x, w, got, EPS, it)
        secs = []
        for _ in range(calls + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = woodbury(At64, x, w, it)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        res[f"torch_woodbury_iter{it}_seconds_median"] = med(secs[1:])
        res[f"library_against_torch_iter{it}_max_abs_diff_of_w2"] = float((got ** 2 - want ** 2).abs().max())
        res[f"iter{it}_max_w2"] = float((want ** 2).max())
    d.close()
    return res


def mode_solve(calls):
    import torch
    cs = load()
    g = torch.Generator(device="cuda").manual_seed(11)
    k = 256
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(torch.float32).contiguous()
    S = torch.randperm(N, generator=g, device="cuda")[:k]
    xs = torch.zeros(N, dtype=torch.float64, device="cuda")
    xs[S] = torch.where(torch.rand(k, generator=g, device="cuda") < 0.5, -1.0, 1.0).to(torch.float64)
    A64 = At.to(torch.float64)
    b = (xs @ A64 + 5e-3 * torch.randn(M, generator=g, device="cuda", dtype=torch.float64)).to(torch.float32)
    v = torch.randn(N, generator=g, device="cuda", dtype=torch.float64)
    for _ in range(40):  # ||A||_2^2 by power iteration
        v = A64 @ (v @ A64)
        s = v.norm()
        v /= s
    alpha, lam = 0.45 / float(s), 0.4  # (reweighting multiplies the penalty by 1 / (|x| + eps): from lambda = 0.5 on a planted +-1 shrinks to zero)
    del A64
    d = cs.Dictionary(At)
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    res = {"mode": "solve", "lambda": lam, "inner_iterations": 256, "outer_solves": 8}
    d.ctx.ista_device(b, lam, x, maxiter=8, stepsize=alpha)  # warm-up
    plain = timed(lambda: [d.ctx.ista_device(b, lam, x, maxiter=256, stepsize=alpha) for _ in range(8)], calls)
    res["ista_8_plain_calls_seconds_median"] = med(plain)
    for scheme in ("candes", "ard"):
        out = []

        def run(outer=8):
            out.append(d.ctx.ista_reweighted_device(b, lam, scheme, x, None, eps=EPS, outer_maxiter=outer, min_decrease=0.0, maxiter=256, stepsize=alpha))

        try:
            run(2)  # warm-up (a shorter inner solve would leave more non-zeros than ARD takes)
            secs = timed(run, calls)
        except cs.CsmpError as e:  # (CSMP_ERANGE: the first solve's support is larger than CSMP_ARD_KMAX)
            res[f"ista_{scheme}_error"] = str(e)
            continue
        res[f"ista_{scheme}_seconds_median"] = med(secs)
        res[f"ista_{scheme}_resnorm"], res[f"ista_{scheme}_nnz"] = out[-1][0], int((x != 0).sum())
        res[f"ista_{scheme}_support_is_planted"] = bool(torch.equal(torch.nonzero(x).flatten(), torch.sort(S).values))
    d.ctx.ista_device(b, lam, x, maxiter=256, stepsize=alpha)
    res["ista_plain_nnz_after_256"] = int((x != 0).sum())
    d.close()
    return res


def mode_once(k):
    import numpy as np
    import torch
    cs = load()
    At, x, w = make_inputs(k)
    d = cs.Dictionary(At)
    d.ctx.ard_weights_device(x, w, torch.empty_like(w), EPS, 1)
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


def trace(k, outdir, limit):
    """one rocprofv3 --kernel-trace --stats run of `--mode once` in a process of its own -> {kernel: {calls, total_ns, mean_us}}"""
    os.makedirs(outdir, exist_ok=True)
    child(["--mode", "once", "--k", str(k)], limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--"))
    kernels = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            short = next((q for q in KERNELS if re.search(r"\b%s\b" % q, name)), None)
            if short:
                e = kernels.setdefault(short, {"calls": 0, "total_ns": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += float(row["TotalDurationNs"])
    for e in kernels.values():
        e["mean_us"] = e["total_ns"] / max(e["calls"], 1) / 1e3
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("weights", "torch", "solve", "once", "all"), default="weights")
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--trace-dir", default=os.path.join(HERE, "build", "reweight_trace"), help="where the kernel trace is written")
    a = ap.parse_args()
    if a.mode == "weights":
        print(json.dumps(mode_weights(a.k, a.calls)))
    elif a.mode == "torch":
        print(json.dumps(mode_torch(a.k, a.calls)))
    elif a.mode == "solve":
        print(json.dumps(mode_solve(a.calls)))
    elif a.mode == "once":
        print(json.dumps(mode_once(a.k)))
    else:
        res = {"shape": [M, N, "float32"], "eps": EPS}

        def save():
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)

        for k in (256, 1024):
            res[f"weights_k{k}"] = child(["--mode", "weights", "--k", str(k), "--calls", str(a.calls)], 240)
            res["measured_on"] = res[f"weights_k{k}"]["device"]
            save()
            res[f"torch_k{k}"] = child(["--mode", "torch", "--k", str(k), "--calls", "1"], 300)
            save()
            kern = res[f"kernel_trace_k{k}"] = trace(k, os.path.join(a.trace_dir, f"k{k}"), 240)
            flop = 2.0 * 128 * N * M  # per block of 128 directions against every atom
            f, r = kern.get("k_ard_forms"), kern.get("k_fr_rebuild_lds")
            blocks = (k + 127) // 128
            if f:
                res[f"k_ard_forms_k{k}_us_per_128_directions"] = f["mean_us"] / blocks
                res[f"k_ard_forms_k{k}_flop_per_s"] = flop / (f["mean_us"] / blocks * 1e-6)
            if r:
                res[f"k_fr_rebuild_lds_k{k}_run_us_per_128_directions"] = r["mean_us"]
                res[f"k_fr_rebuild_lds_k{k}_run_flop_per_s"] = flop / (r["mean_us"] * 1e-6)
            save()
        res["solve"] = child(["--mode", "solve", "--calls", str(a.calls)], 300)
        save()
        print(json.dumps({q: v for q, v in res.items() if q.startswith("k_")}))
        for q in ("weights_k256", "weights_k1024", "torch_k256", "torch_k1024", "solve"):
            print(q, json.dumps({u: v for u, v in res[q].items() if not isinstance(v, list)}))


if __name__ == "__main__":
    main()
