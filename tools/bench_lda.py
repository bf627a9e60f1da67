"""Gibbs LDA sweep rate: the fused engine (csrc/gibbs.hip) against its numpy twin, and the
wall time of a whole training run next to Mallet's published figure.

The corpus is the reference generator's centralized one: 5 nodes x 1000 documents, V = 5000,
K = 50, 150-250 tokens a document (data/synthetic.py, seed 0), about a million tokens.
BASELINE.md quotes Mallet at 46 s for 1000 iterations on 5000 documents at K = 50
(notebooks/tests/Centralized-Mallet-Prod.ipynb, the authors' CPU; a figure from the
literature of the project, not a measurement of this tool).

Timings are host clocks around work that ends in a device synchronise:
  cold   the first construction of a sampler in the process (kernel library load, upload,
         inverted index, initial state) and its first sweep
  warm   --reps windows on that sampler, each of as many batches of --window sweeps as it
         takes to fill --min-window seconds: ms per sweep (sweep + recount + nk), median and
         min / max of the windows, and tokens / s from the median
  fit    GibbsLDA.fit with --iterations sweeps and Mallet's optimize_interval = 10 after 200
         burn-in sweeps, once
  twin   --twin-sweeps sweeps of the host engine on the same corpus, each timed

usage: python tools/bench_lda.py [--iterations 1000] [--reps 5] [--min-window 0.5] [--out FILE]
Prints one JSON line and appends it to --out (default profiles/lda_bench.jsonl, which holds
the recorded runs).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gfedntm_amd.data.bow import DeviceCSR  # noqa: E402
from gfedntm_amd.data.synthetic import generate_synthetic  # noqa: E402
from gfedntm_amd.models import GibbsLDA  # noqa: E402
from gfedntm_amd.ops import lda  # noqa: E402

MALLET_S = 46.0          # 1000 iterations, 5000 documents, K = 50


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--min-window", type=float, default=0.5)
    ap.add_argument("--twin-sweeps", type=int, default=3)
    ap.add_argument("--topics", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lda_bench.jsonl"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lda needs a GPU: the fused engine is what it measures")
    syn = generate_synthetic(vocab_size=5000, n_topics=50, n_docs=1000, n_nodes=5, seed=0)
    X = sp.vstack(syn.counts).tocsr()
    K, alpha_k, beta = a.topics, 5.0 / a.topics, 0.01
    tokens = int(X.sum())

    (s, t_setup) = clock(lambda: lda.GibbsSampler(DeviceCSR(X, "cuda:0"), K, alpha_k, beta, seed=0))
    _, t_first = clock(s.sweep)
    warm, n_win = [], 0
    for _ in range(a.reps):
        n, t = 0, 0.0
        while t < a.min_window:
            t += clock(lambda: s.sweep(a.window))[1]
            n += a.window
        warm.append(1e3 * t / n)
        n_win = n
    med = statistics.median(warm)

    m = GibbsLDA(K, alpha=5.0, beta=beta, num_iterations=a.iterations, optimize_interval=10,
                 burn_in=200, seed=0, device="cuda:0")
    _, t_fit = clock(lambda: m.fit(DeviceCSR(X, "cuda:0")))
    phi = m.get_topic_word_distribution()
    match = float((np.sqrt(syn.topic_vectors) @ np.sqrt(phi).T).max(1).mean()) if K == 50 else None

    h = lda.GibbsSampler(X, K, alpha_k, beta, seed=0, engine="host")
    twin = []
    for _ in range(a.twin_sweeps):
        t0 = time.perf_counter()
        h.sweep()
        twin.append(1e3 * (time.perf_counter() - t0))
    tmed = statistics.median(twin)

    rec = {"bench": "lda", "device": torch.cuda.get_device_name(0), "docs": int(X.shape[0]),
           "V": int(X.shape[1]), "K": K, "tokens": tokens, "nnz": int(X.nnz),
           "cold_setup_s": round(t_setup, 4), "cold_first_sweep_ms": round(1e3 * t_first, 3),
           "warm_sweep_ms": round(med, 4), "warm_sweep_ms_min": round(min(warm), 4),
           "warm_sweep_ms_max": round(max(warm), 4), "warm_windows": a.reps,
           "sweeps_in_last_window": n_win, "fused_tokens_per_s": round(tokens / (med * 1e-3)),
           "fit_iterations": a.iterations, "fit_wall_s": round(t_fit, 3),
           "fit_optimize_interval": 10, "fit_topic_match": match,
           "mallet_published_s_per_1000_iterations": MALLET_S,
           "twin_sweep_ms": round(tmed, 2), "twin_sweeps": a.twin_sweeps,
           "twin_tokens_per_s": round(tokens / (tmed * 1e-3)),
           "fused_over_twin": round(tmed / med, 1)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
