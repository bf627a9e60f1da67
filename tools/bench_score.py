"""Held-out scoring throughput: the fused path (csrc/score.hip through ``tm.score``:
encoder once per document, eval-mode decoder on the matrix cores, no dense rows) vs the
PyTorch path of the same model (``engine="torch"``: the eval-mode modules over dense
[chunk, V] rows), same GPU, one draw per document (the validation estimator), interleaved.

The two shapes are the README's ProdLDA ones: K = 50 V = 4466 and K = 200 V = 112k.
``--model LDA`` times the NeuralLDA decoder on the same shapes (``engine="fused"`` there is
the sparse-only scorer: a per-topic log-sum-exp once per call and the non-zeros; the default
engine of such a model is still the PyTorch path).

usage: python tools/bench_score.py [--shape small|large|both] [--model prodLDA|LDA] [--reps 7]
                                   [--out FILE]
Prints one JSON line per shape (docs/s of each path: the median of --reps windows, and the
spread), appended to --out when given.
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

from gfedntm_amd.data.bow import BatchPlan, BOWDataset  # noqa: E402
from gfedntm_amd.data.synthetic import generate_synthetic, remap_to_vocabulary  # noqa: E402
from gfedntm_amd.models import AVITM  # noqa: E402

SHAPES = {   # K, V, hidden, documents scored, documents generated (tiled up to the former)
    "small": dict(K=50, V=4466, hidden=(50, 50), docs=20000, base=2000),
    "large": dict(K=200, V=112000, hidden=(50, 50), docs=4096, base=512),
}


def window(fn, min_s=0.25):
    """docs-independent timing window: repeat ``fn`` until at least ``min_s`` seconds of
    synchronised work; returns seconds per call."""
    n, t = 0, 0.0
    t0 = time.perf_counter()
    while t < min_s:
        fn()
        torch.cuda.synchronize()
        n += 1
        t = time.perf_counter() - t0
    return t / n


def run(name, cfg, reps, steps, model_type="prodLDA"):
    dev = torch.device("cuda")
    K, V = cfg["K"], cfg["V"]
    corpus = generate_synthetic(vocab_size=V, n_topics=K, n_docs=cfg["base"], n_nodes=1,
                                frozen_topics=5, seed=0)
    X = remap_to_vocabulary(corpus, 0, {f"wd{i}": i for i in range(V)})
    X = sp.vstack([X] * (-(-cfg["docs"] // cfg["base"]))).tocsr()[: cfg["docs"]]
    tm = AVITM(input_size=V, n_components=K, model_type=model_type, hidden_sizes=cfg["hidden"], batch_size=64,
               verbose=False, device=dev, backend="fused", seed=0)
    ds = BOWDataset(X, None)
    data = tm.device_data(ds)
    tm.engine.bind_data(data, BatchPlan.build(data.n_docs, 64, steps, seed=0))
    for s in range(steps):                   # a few steps: non-trivial weights and statistics
        tm.engine.step(s)
    torch.cuda.synchronize()

    paths = {"fused": lambda: tm.score(ds, n_samples=1, seed=3, engine="fused"),
             "torch": lambda: tm.score(ds, n_samples=1, seed=3, engine="torch")}
    res = {k: f() for k, f in paths.items()}          # warm-up of every shape timed below
    res = {k: f() for k, f in paths.items()}
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(reps):                             # interleaved
        for k, f in paths.items():
            times[k].append(window(f))
    n = data.n_docs
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"metric": "held-out scoring docs/s (1 draw per document)", "shape": name, "model": model_type,
           "K": K, "V": V,
           "docs": n, "nnz": int(data.nnz), "reps": reps,
           "fused_docs_per_s": round(n / med["fused"], 1), "fused_ms": round(med["fused"] * 1e3, 3),
           "fused_ms_min_max": [round(min(times["fused"]) * 1e3, 3), round(max(times["fused"]) * 1e3, 3)],
           "torch_docs_per_s": round(n / med["torch"], 1), "torch_ms": round(med["torch"] * 1e3, 3),
           "torch_ms_min_max": [round(min(times["torch"]) * 1e3, 3), round(max(times["torch"]) * 1e3, 3)],
           "speedup": round(med["torch"] / med["fused"], 2),
           # same weights: KL has no draw in it; the RL means differ by their draws only
           "kl_max_abs_diff": float(np.abs(res["fused"]["kl"] - res["torch"]["kl"]).max()),
           "loss_fused": round(res["fused"]["loss"], 4), "loss_torch": round(res["torch"]["loss"], 4),
           "perplexity_fused": round(res["fused"]["perplexity"], 3),
           "perplexity_torch": round(res["torch"]["perplexity"], 3)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", default="both", choices=["small", "large", "both"])
    p.add_argument("--model", default="prodLDA", choices=["prodLDA", "LDA"])
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--steps", type=int, default=20, help="training steps before scoring")
    p.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score needs a GPU")
    for name in (["small", "large"] if a.shape == "both" else [a.shape]):
        line = json.dumps(run(name, SHAPES[name], a.reps, a.steps, a.model))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
