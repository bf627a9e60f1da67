"""TSS / DSS time: the device path (operands resident on the GPU -> csrc/simscore.hip float64
tiles -> one scalar read back) vs the host formula of eval/metrics.py (numpy, two dense
[D, D] float64 matrices for DSS) on the same inputs, interleaved.

DSS at (D, K) = (5 000, 50) and (50 000, 50): thetas_true ~ Dirichlet(0.1), thetas ~
Dirichlet(0.1) thresholded at 3e-3 and renormalised.  TSS at (K, V) = (50, 4 466) and
(200, 100 000): Dirichlet(0.01) topics, the learned side zero on an eighth of the columns.
At D = 50 000 the host formula needs 2 x 20 GB and is not run; the record says so.

usage: python tools/bench_simscore.py [--only dss|tss] [--reps 5] [--out FILE]
Prints one JSON line per config (ms of each path: the median of --reps windows and their
min / max, the two results and their difference, peak device bytes), appended to --out when
given (profiles/simscore_bench.jsonl holds the recorded runs).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gfedntm_amd.eval import metrics  # noqa: E402

DSS_SHAPES = [(5000, 50), (50000, 50)]
TSS_SHAPES = [(50, 4466), (200, 100000)]
HOST_BYTES_CAP = 8 << 30        # the host formula is run while its two matrices stay below this


def window(fn, min_s=0.25):
    """Repeat ``fn`` until at least ``min_s`` seconds of synchronised work; seconds per call."""
    n, t = 0, 0.0
    t0 = time.perf_counter()
    while t < min_s:
        fn()
        torch.cuda.synchronize()
        n += 1
        t = time.perf_counter() - t0
    return t / n


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def measure(out, paths, reps):
    res = {k: f() for k, f in paths.items()}              # warm-up of every path timed below
    res = {k: f() for k, f in paths.items()}
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(reps):                                 # interleaved
        for k, f in paths.items():
            times[k].append(window(f))
    for k in paths:
        out[f"{k}_ms"] = round(statistics.median(times[k]) * 1e3, 3)
        out[f"{k}_ms_min_max"] = [round(min(times[k]) * 1e3, 3), round(max(times[k]) * 1e3, 3)]
        out[k] = res[k]
    out["device_peak_device_bytes"] = peak_bytes(paths["device"])
    if "host" in paths:
        out["speedup"] = round(out["host_ms"] / out["device_ms"], 2)
        out["abs_diff"] = abs(res["device"] - res["host"])
    return out


def run_dss(D, K, reps):
    rng = np.random.default_rng(0)
    tt = rng.dirichlet([0.1] * K, D)
    th = rng.dirichlet([0.1] * K, D)
    th[th < 3e-3] = 0.0
    th /= th.sum(1, keepdims=True)
    dtt, dth = torch.from_numpy(tt).cuda(), torch.from_numpy(th).cuda()
    out = {"metric": "DSS ms per call (float64)", "D": D, "K": K, "reps": reps,
           "flops": 2 * 2 * K * (D * (D + 1) // 2)}
    paths = {"device": lambda: metrics.dss(dtt, dth, engine="device")}
    host_bytes = 2 * 8 * D * D
    if host_bytes <= HOST_BYTES_CAP:
        paths["host"] = lambda: metrics.dss(tt, th, engine="host")
    else:
        out["host_ms"] = None
        out["host_not_run"] = (f"the host formula builds two float64 [D, D] matrices: "
                               f"2 x {8 * D * D / 1e9:.1f} GB at D = {D}")
    out = measure(out, paths, reps)
    out["device_tflops"] = round(out["flops"] / (out["device_ms"] * 1e-3) / 1e12, 3)
    return out


def run_tss(K, V, reps):
    rng = np.random.default_rng(1)
    gt = rng.dirichlet([0.01] * V, K)
    b = rng.dirichlet([0.01] * V, K)
    b[:, rng.choice(V, V // 8, replace=False)] = 0.0
    s = b.sum(1, keepdims=True)
    s[s == 0] = 1.0
    b /= s
    db, dgt = torch.from_numpy(b).cuda(), torch.from_numpy(gt).cuda()
    out = {"metric": "TSS ms per call (float64)", "K": K, "V": V, "reps": reps}
    paths = {"device": lambda: metrics.tss(db, dgt, engine="device"),
             "host": lambda: metrics.tss(b, gt, engine="host")}
    return measure(out, paths, reps)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--only", default=None, choices=["dss", "tss"])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simscore needs a GPU")
    jobs = []
    if a.only != "tss":
        jobs += [lambda s=s: run_dss(*s, a.reps) for s in DSS_SHAPES]
    if a.only != "dss":
        jobs += [lambda s=s: run_tss(*s, a.reps) for s in TSS_SHAPES]
    for job in jobs:
        line = json.dumps(job())
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
