"""csmp_mp_batch against the caller's loop over csmp_mp, at the benchmark's shape (4096 x 65536 Float32, k = 256).

    python tools/bench_mp_batch.py --mode batch            # this tree: csmp_mp_batch, nsig in (1, 2, 4, 8, 16, 18, 32)
    python tools/bench_mp_batch.py --mode loop [--root D]  # the loop of csmp_mp over the same signals (D: another built checkout)
    python tools/bench_mp_batch.py --mode ab --baseline-root D [--rounds 2] [--out profiles/r10_mp_batch.json]

ab alternates fresh child processes -- the loop on the baseline checkout D (the parent commit, built), the batch on this tree -- and
prints the comparison: atoms/s of the batch at nsig = 16 over atoms/s of the baseline's loop, beside the prediction
8 / (a wide 4 + 4 pass in narrow passes), re-measured in the same session with csmp_bench_sweep variants 1 and 3.
Per nsig: a warm-up call, then `--calls` timed calls; atoms/s by the host clock around the call (the batch: device pointers in and
out, ended by csmp_sync; the loop: csmp_mp on a host signal, as its C ABI has it), and for the batch the window of its timed passes
(csmp_profile_window), taken in a further call.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSIGS = (1, 2, 4, 8, 16, 18, 32)
M, N = 4096, 65536


def make_inputs(nsig):
    """the dictionary (unit-norm Gaussian atoms, generated on the device) and nsig planted 16-sparse signals with noise"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(2024)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(torch.float32)
    atoms = torch.randint(0, N, (nsig, 16), generator=g, device="cuda")
    signs = torch.randint(0, 2, (nsig, 16), generator=g, device="cuda").to(torch.float64) * 2 - 1
    B = (At[atoms].to(torch.float64) * signs[:, :, None]).sum(dim=1)
    e = torch.randn((nsig, M), generator=g, device="cuda", dtype=torch.float64)
    B += e * (5e-2 / e.norm(dim=1, keepdim=True))
    return At, B.contiguous()


def measure(mode, root, k, calls, nsigs):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from csmp_pkg import load
    cs = load()
    At, B = make_inputs(max(nsigs))
    d = cs.Dictionary(At)
    Bh = np.ascontiguousarray(B.cpu().numpy())
    out = {"mode": mode, "root": os.path.basename(os.path.abspath(root)), "k": k, "calls": calls, "device": d.ctx.device_info()[0], "rows": []}
    if mode == "batch":
        narrow, wide = d.ctx.bench_sweep(1, 20), d.ctx.bench_sweep(3, 20)
        out["sweep_ms"] = {"narrow_4": narrow, "wide_4_4": wide, "wide_in_narrow_passes": wide / narrow, "prediction": 8.0 / (wide / narrow)}
    for nsig in nsigs:
        row = {"nsig": nsig}
        if mode == "loop":
            def call():
                for s in range(nsig):
                    d.ctx.mp(Bh[s], k)
        else:
            idx = torch.empty((nsig, k), dtype=torch.int64, device="cuda")
            val = torch.empty((nsig, k), dtype=torch.float64, device="cuda")
            nnz = torch.empty((nsig,), dtype=torch.int64, device="cuda")
            Bd = B[:nsig].contiguous()
            fn = d.ctx.omp_batch_device if mode == "omp_batch" else d.ctx.mp_batch_device
            args = (Bd, k, 1e-9, idx, val, nnz) if mode == "omp_batch" else (Bd, k, idx, val, nnz)

            def call():
                fn(*args)
                d.ctx.sync()
        call()  # warm-up: slots, the twin, code objects
        times = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        row["seconds"] = times
        row["atoms_per_s"] = [nsig * k / t for t in times]
        row["atoms_per_s_median"] = sorted(row["atoms_per_s"])[len(times) // 2]
        if mode != "loop":
            d.ctx.profile_enable(True)
            d.ctx.profile_read(reset=True)
            call()
            row["pass_window"] = d.ctx.profile_window()
            d.ctx.profile_read(reset=True)
            d.ctx.profile_enable(False)
        if mode == "batch":  # the batch's results are the loop's
            got = (idx.cpu().numpy(), val.cpu().numpy(), nnz.cpu().numpy())
            for s in sorted({0, nsig - 1}):
                i, v = d.ctx.mp(Bh[s], k)
                assert got[2][s] == len(i) and np.array_equal(got[0][s, :len(i)], i) and np.array_equal(got[1][s, :len(i)], v), (nsig, s)
            row["checked_against_csmp_mp"] = True
        out["rows"].append(row)
    d.close()
    return out


def child(mode, root, k, calls, nsigs):
    cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--root", root, "--k", str(k), "--calls", str(calls),
           "--nsig", ",".join(map(str, nsigs))]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{mode} on {root} failed ({p.returncode})")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("batch", "loop", "omp_batch", "ab"), default="batch")
    ap.add_argument("--root", default=HERE, help="the built checkout to measure (default: this tree)")
    ap.add_argument("--baseline-root", help="ab: a built checkout of the parent commit")
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nsig", default=",".join(map(str, NSIGS)))
    ap.add_argument("--out")
    a = ap.parse_args()
    nsigs = tuple(int(x) for x in a.nsig.split(","))
    if a.mode != "ab":
        print(json.dumps(measure(a.mode, a.root, a.k, a.calls, nsigs)))
        return
    if not a.baseline_root:
        raise SystemExit("--mode ab needs --baseline-root")
    runs = []
    for _ in range(a.rounds):  # builds alternated in one session
        runs.append(child("loop", a.baseline_root, a.k, a.calls, nsigs))
        runs.append(child("batch", a.root, a.k, a.calls, nsigs))
    runs.append(child("omp_batch", a.root, a.k, a.calls, (16,)))
    med = lambda v: sorted(v)[len(v) // 2]
    table = {}
    for nsig in nsigs:
        loop = [x for r in runs if r["mode"] == "loop" for row in r["rows"] if row["nsig"] == nsig for x in row["atoms_per_s"]]
        batch = [x for r in runs if r["mode"] == "batch" for row in r["rows"] if row["nsig"] == nsig for x in row["atoms_per_s"]]
        table[nsig] = {"loop_atoms_per_s": med(loop), "loop_min_max": [min(loop), max(loop)], "batch_atoms_per_s": med(batch),
                       "batch_min_max": [min(batch), max(batch)], "ratio": med(batch) / med(loop)}
    pred = med([r["sweep_ms"]["prediction"] for r in runs if r["mode"] == "batch"])
    res = {"shape": [M, N, "float32"], "k": a.k, "baseline": "the parent commit: a loop of csmp_mp over the same signals",
           "compared": "atoms/s of csmp_mp_batch at nsig = 16 over atoms/s of the baseline's loop",
           "ratio_nsig_16": table[16]["ratio"] if 16 in table else None, "prediction": pred, "bar": pred / 2, "table": table, "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({kk: res[kk] for kk in ("ratio_nsig_16", "prediction", "bar")}))
    for nsig in nsigs:
        print(nsig, json.dumps(table[nsig]))


if __name__ == "__main__":
    main()
