"""HTM-WS submodel corpus and document-completion split time: the keyed paths
(csrc/thin.hip through gfedntm_amd/ops/thin.py) vs the existing
``htm_ws_counts(device="cuda")`` (chunks of 2^20 non-zeros: upload, a [chunk, K] gather of
beta, ``torch.binomial``, copy back) on the same corpus, thetas, betas and GPU, interleaved.

  torch           htm_ws_counts(X, ..., device="cuda")                 scipy in, scipy out
  keyed           htm_ws_counts(X, ..., device="cuda", engine="keyed") scipy in, scipy out
  keyed_resident  thin_by_topic on the resident DeviceCSR (theta / beta on the device),
                  the result left on the device
  split           split(DeviceCSR, 0.5): both parts, left on the device

Two shapes (those of tools/bench_cooc.py): K = 50, V = 4466, 20 000 documents, and
K = 200, V = 100k, 200 000 documents.

usage: python tools/bench_thin.py [--shape small|large|both] [--reps 5] [--out FILE]
Prints one JSON line per shape (ms of each path: the median of --reps windows and their
min / max), appended to --out when given (profiles/thin_bench.jsonl holds the recorded
runs).
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
from gfedntm_amd.experiments.tm_wrapper import htm_ws_counts  # noqa: E402
from gfedntm_amd.ops import thin  # noqa: E402

SHAPES = {   # K, V, documents, documents generated (tiled up to the former)
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


def run(name, cfg, reps):
    K, V, topic = cfg["K"], cfg["V"], 1
    corpus = generate_synthetic(vocab_size=V, n_topics=K, n_docs=cfg["base"], n_nodes=1,
                                frozen_topics=5, seed=0)
    X = remap_to_vocabulary(corpus, 0, {f"wd{i}": i for i in range(V)})
    X = sp.vstack([X] * (-(-cfg["docs"] // cfg["base"]))).tocsr()[: cfg["docs"]]
    X.sort_indices()
    rng = np.random.default_rng(1)
    thetas = rng.dirichlet(np.full(K, 0.1), size=X.shape[0]).astype(np.float32)
    z = rng.standard_normal((K, V)).astype(np.float32) * 2.0
    betas = np.exp(z - z.max(1, keepdims=True))
    betas /= betas.sum(1, keepdims=True)
    data = DeviceCSR(X, "cuda")
    th_dev, be_dev = torch.from_numpy(thetas).cuda(), torch.from_numpy(betas).cuda()

    paths = {
        "torch": lambda: htm_ws_counts(X, thetas, betas, topic, seed=0, device="cuda"),
        "keyed": lambda: htm_ws_counts(X, thetas, betas, topic, seed=0, device="cuda", engine="keyed"),
        "keyed_resident": lambda: thin.thin_by_topic(data, th_dev, be_dev, topic, 0),
        "split": lambda: thin.split(data, 0.5, 0),
    }
    res = {k: f() for k, f in paths.items()}          # warm-up of every shape timed below
    res = {k: f() for k, f in paths.items()}
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(reps):                             # interleaved
        for k, f in paths.items():
            times[k].append(window(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"metric": "HTM-WS submodel corpus / completion split, ms per call", "shape": name,
           "K": K, "V": V, "D": int(X.shape[0]), "nnz": int(X.nnz), "tokens": int(X.sum()),
           "reps": reps}
    for k in paths:
        out[f"{k}_ms"] = round(med[k] * 1e3, 3)
        out[f"{k}_ms_min_max"] = [round(min(times[k]) * 1e3, 3), round(max(times[k]) * 1e3, 3)]
    out["speedup_keyed"] = round(med["torch"] / med["keyed"], 2)
    out["speedup_keyed_resident"] = round(med["torch"] / med["keyed_resident"], 2)
    # the two draws differ, their law does not: kept tokens of each path
    out["kept_tokens_torch"] = int(res["torch"].sum())
    out["kept_tokens_keyed"] = int(res["keyed"].sum())
    kr = res["keyed_resident"]
    out["keyed_equals_resident"] = bool(
        np.array_equal(res["keyed"].indptr, kr.indptr.cpu().numpy())
        and np.array_equal(res["keyed"].indices, kr.indices.cpu().numpy())
        and np.array_equal(res["keyed"].data, kr.values.cpu().numpy()))
    k, r = res["split"]
    out["split_tokens"] = [int(k.values.sum().item()), int(r.values.sum().item())]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", default="both", choices=["small", "large", "both"])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_thin needs a GPU")
    for name in (["small", "large"] if a.shape == "both" else [a.shape]):
        line = json.dumps(run(name, SHAPES[name], a.reps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
