"""NPMI coherence time: the fused path (the corpus already resident as a DeviceCSR ->
csrc/cooc.hip integer co-occurrence counts -> float64 NPMI on the host) vs the dense path
``npmi_coherence(..., device="cuda")`` (host column slice + densify [D, W] fp32 + upload +
library GEMM) on the same corpus, topics and GPU, interleaved.

Two shapes: the bench's K = 50, V = 4466, top-10 over 20 000 documents, and K = 200,
V = 100k, top-10 over 200 000 documents.  The topics' words are drawn (seeded) from the
most frequent vocabulary words, so W is close to K * 10.

usage: python tools/bench_cooc.py [--shape small|large|both] [--reps 5] [--out FILE]
Prints one JSON line per shape (ms of each path: the median of --reps windows and their
min / max, W, D, peak device bytes of each path), appended to --out when given
(profiles/cooc_bench.jsonl holds the recorded runs).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gfedntm_amd.data.bow import DeviceCSR  # noqa: E402
from gfedntm_amd.data.synthetic import generate_synthetic, remap_to_vocabulary  # noqa: E402
from gfedntm_amd.eval.metrics import (cooccurrence_counts, npmi_coherence,  # noqa: E402
                                      npmi_from_counts)

SHAPES = {   # K, V, documents scored, documents generated (tiled up to the former)
    "small": dict(K=50, V=4466, docs=20000, base=2000),
    "large": dict(K=200, V=100000, docs=200000, base=2000),
}


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


def run(name, cfg, reps):
    K, V, topk = cfg["K"], cfg["V"], 10
    corpus = generate_synthetic(vocab_size=V, n_topics=K, n_docs=cfg["base"], n_nodes=1,
                                frozen_topics=5, seed=0)
    X = remap_to_vocabulary(corpus, 0, {f"wd{i}": i for i in range(V)})
    X = sp.vstack([X] * (-(-cfg["docs"] // cfg["base"]))).tocsr()[: cfg["docs"]]
    X.sort_indices()
    df = np.asarray((X > 0).sum(0)).ravel()
    pool = np.argsort(-df, kind="stable")[: max(K * topk * 2, 1000)]
    rng = np.random.default_rng(1)
    topics = [list(map(int, rng.choice(pool, size=topk, replace=False))) for _ in range(K)]
    words = sorted({w for t in topics for w in t})
    data = DeviceCSR(X, "cuda")
    wdev = torch.tensor(words, device="cuda")
    n_docs = X.shape[0]

    def fused():
        counts = cooccurrence_counts(data, wdev, engine="fused")
        return npmi_from_counts(topics, words, counts, n_docs, per_topic=True)

    def dense():
        return npmi_coherence(topics, X, per_topic=True, device="cuda")

    paths = {"fused": fused, "dense": dense}
    res = {k: f() for k, f in paths.items()}          # warm-up of every shape timed below
    res = {k: f() for k, f in paths.items()}
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(reps):                             # interleaved
        for k, f in paths.items():
            times[k].append(window(f))
    peaks = {k: peak_bytes(f) for k, f in paths.items()}
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"metric": "NPMI coherence ms per call (top-10 words)", "shape": name, "K": K, "V": V,
           "D": int(n_docs), "W": len(words), "nnz": int(X.nnz), "reps": reps}
    for k in paths:
        out[f"{k}_ms"] = round(med[k] * 1e3, 3)
        out[f"{k}_ms_min_max"] = [round(min(times[k]) * 1e3, 3), round(max(times[k]) * 1e3, 3)]
        out[f"{k}_peak_device_bytes"] = peaks[k]
    out["speedup"] = round(med["dense"] / med["fused"], 2)
    # the same float64 formula on the same integers
    out["per_topic_max_abs_diff"] = float(np.abs(np.array(res["fused"]) - np.array(res["dense"])).max())
    out["npmi"] = round(float(np.mean(res["fused"])), 6)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", default="both", choices=["small", "large", "both"])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cooc needs a GPU")
    for name in (["small", "large"] if a.shape == "both" else [a.shape]):
        line = json.dumps(run(name, SHAPES[name], a.reps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
