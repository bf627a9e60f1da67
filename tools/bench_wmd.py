"""Mean-min WMD time of one table cell: the device path (word vectors resident on the GPU ->
csrc/wmd.hip distances + batched exact transport -> one copy back) vs the numpy twin of the
same solver ("host") and today's default, one scipy LP per topic pair ("lp"), on the same
topics, interleaved.

A cell compares K_ref = 50 reference topics with K_cmp = 50 topics: 2 500 transport problems.
Topics are synthetic word lists over 300-dimensional unit vectors; a compared topic shares
about a third of its words with the reference topic of the same index.  Shapes: n_words in
{10, 100, 300} on both sides, and 300 against 287 words (coprime lengths: T = n m units flow).

The device path is always timed on the full cell.  The host twin is timed on the full cell
while one pass stays below --full-budget seconds; beyond that, and for the LP path always, a
sample of --sample problems is timed, reported per problem and extrapolated to the cell (the
record says which: at 300 words the full LP cell is hours of work).  A path whose one pass takes
more than 2 s is timed by that one pass instead of --reps windows; the record holds the count.

usage: python tools/bench_wmd.py [--only 10,100,300,287] [--reps 5] [--sample 20] [--out FILE]
Prints one JSON line per shape (ms per cell of each path: the median of its windows and their
min / max; per-problem ms of the sampled paths; the worst difference between the paths on the
sample; peak device bytes), appended to --out when given (profiles/wmd_bench.jsonl holds the
recorded runs).
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

K_REF = K_CMP = 50
DIM = 300
VOCAB = 20000
SHAPES = {"10": (10, 10), "100": (100, 100), "300": (300, 300), "287": (300, 287)}


def topics(n_ref, n_cmp, seed):
    """(reference topics, compared topics, word vectors): compared topic k repeats a third of
    reference topic k's words."""
    rng = np.random.default_rng(seed)
    words = [f"w{i}" for i in range(VOCAB)]
    v = rng.standard_normal((VOCAB, DIM))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ref = [[words[i] for i in rng.choice(VOCAB, n_ref, replace=False)] for _ in range(K_REF)]
    cmp_ = []
    for k in range(K_CMP):
        shared = ref[k % K_REF][:n_cmp // 3]
        taken = set(shared)
        rest = [w for w in (words[i] for i in rng.choice(VOCAB, n_cmp + len(shared), replace=False))
                if w not in taken][:n_cmp - len(shared)]
        cmp_.append(shared + rest)
    return ref, cmp_, dict(zip(words, v))


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


def run(name, reps, sample, full_budget):
    n_ref, n_cmp = SHAPES[name]
    ref, cmp_, vec = topics(n_ref, n_cmp, seed=n_ref + n_cmp)
    nw = max(n_ref, n_cmp)
    cmp_ = [t[:n_cmp] for t in cmp_]
    used = [w for t in ref + cmp_ for w in t]
    dev_table = metrics.WordTable(vec, used, device=True)          # uploaded once per table
    host_table = metrics.WordTable(vec, used)
    n_prob = K_REF * K_CMP
    out = {"metric": "mean-min WMD, ms per cell (float64, exact)", "K_ref": K_REF, "K_cmp": K_CMP,
           "n_words": [n_ref, n_cmp], "dim": DIM, "problems": n_prob, "reps": reps}
    rng = np.random.default_rng(1)
    pairs = [(int(i), int(j)) for i, j in zip(rng.integers(0, K_REF, sample), rng.integers(0, K_CMP, sample))]

    def device():
        return metrics.mean_min_wmd(ref, cmp_, dev_table, nw, engine="device")

    def host_full():
        return metrics.mean_min_wmd(ref, cmp_, host_table, nw, engine="host")

    def host_sample():
        return [metrics.word_movers_distance(ref[i], cmp_[j], host_table, engine="host") for i, j in pairs]

    def lp_sample():
        return [metrics.word_movers_distance(ref[i], cmp_[j], vec) for i, j in pairs]

    def device_sample():
        return [metrics.word_movers_distance(ref[i], cmp_[j], dev_table, engine="device") for i, j in pairs]

    # one pass of each sampled path: its cost decides how it is timed, its values are compared
    res, first = {}, {}
    for key, fn in (("device_sample", device_sample), ("host_sample", host_sample), ("lp_sample", lp_sample)):
        t0 = time.perf_counter()
        res[key] = fn()
        first[key] = time.perf_counter() - t0
    host_is_full = first["host_sample"] / sample * n_prob <= full_budget
    paths = {"device": device, "host": host_full if host_is_full else host_sample, "lp": lp_sample}
    res["device"] = device()                                       # warm-up of the full cell
    torch.cuda.synchronize()
    if host_is_full:
        t0 = time.perf_counter()
        res["host"] = host_full()
        first["host"] = time.perf_counter() - t0
    cost = {"device": 0.0, "host": first["host"] if host_is_full else first["host_sample"],
            "lp": first["lp_sample"]}
    times = {k: [] for k in paths}
    for r in range(reps):                                          # interleaved
        for k, f in paths.items():
            if cost[k] <= 2.0:
                times[k].append(window(f))
            elif r == 0:                                           # a long pass: the one already made
                times[k].append(cost[k])
    scale = {"device": 1.0, "host": 1.0 if host_is_full else n_prob / sample, "lp": n_prob / sample}
    for k in paths:
        ms = [t * 1e3 * scale[k] for t in times[k]]
        out[f"{k}_ms"] = round(statistics.median(ms), 3)
        out[f"{k}_ms_min_max"] = [round(min(ms), 3), round(max(ms), 3)]
        out[f"{k}_windows"] = len(ms)
    out["host_timed_on"] = "the full cell" if host_is_full else f"{sample} problems, extrapolated"
    out["lp_timed_on"] = f"{sample} problems, extrapolated"
    out["lp_ms_per_problem"] = round(out["lp_ms"] / n_prob, 3)
    out["host_ms_per_problem"] = round(out["host_ms"] / n_prob, 3)
    out["device_ms_per_problem"] = round(out["device_ms"] / n_prob, 5)
    if out["lp_ms"] > 600e3:
        out["lp_note"] = f"the full LP cell would take {out['lp_ms'] / 3.6e6:.1f} hours and is not run"
    out["mean_min_wmd_device"] = res["device"]
    if host_is_full:
        out["mean_min_wmd_host"] = res["host"]
    out["sample_abs_diff_device_host"] = float(np.max(np.abs(np.subtract(res["device_sample"], res["host_sample"]))))
    out["sample_abs_diff_device_lp"] = float(np.max(np.abs(np.subtract(res["device_sample"], res["lp_sample"]))))
    out["speedup_vs_host"] = round(out["host_ms"] / out["device_ms"], 2)
    out["speedup_vs_lp"] = round(out["lp_ms"] / out["device_ms"], 2)
    out["device_peak_device_bytes"] = peak_bytes(device)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--only", default="10,100,300,287", help="shapes: 10, 100, 300, 287 (= 300 x 287)")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--sample", type=int, default=20)
    p.add_argument("--full-budget", type=float, default=20.0,
                   help="seconds one full-cell pass of the host twin may take")
    p.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wmd needs a GPU")
    for name in a.only.split(","):
        line = json.dumps(run(name, a.reps, a.sample, a.full_budget))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
