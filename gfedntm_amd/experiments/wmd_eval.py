"""Word-mover's distances between non-collaborative (node) models and every model.

Reference: aux_scripts/evaluation/wmd.py:13-110 -- for each K, a [nodes x all
models] table of mean over the node model's topics of the minimum WMD to the
other model's topics, on the top ``n_words`` words, one CSV per (K, n_words).
The reference loads word2vec-google-news-300 through gensim's downloader; there
is no network here, so the word vectors are given as a file: word2vec text
format (``word v1 v2 ...`` per line, optional header) or an ``.npz`` with
``words`` and ``vectors`` arrays.  Vectors are L2-normalised like gensim's
``init_sims(replace=True)``.  Model folders are the ones written by
:mod:`gfedntm_amd.experiments.collab` (``topics.json``).

``engine``: None / "lp" -- one LP per topic pair (eval/metrics.py word_movers_distance);
"host" / "device" -- every cell's [K_ref, K_cmp] problems as one batch of the exact transport
solver (ops/wmd.py numpy twin / csrc/wmd.hip kernels); with "device" the vectors of a table's
words are uploaded once per table and every cell gathers from that copy.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Optional

import numpy as np

from ..eval.metrics import WordTable, mean_min_wmd


def load_vectors(path: str) -> Dict[str, np.ndarray]:
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            words, vecs = [str(w) for w in z["words"]], np.asarray(z["vectors"], dtype=np.float64)
    else:
        words, rows = [], []
        with open(path, encoding="utf8") as f:
            for i, line in enumerate(f):
                parts = line.rstrip().split(" ")
                if i == 0 and len(parts) == 2 and all(p.isdigit() for p in parts):
                    continue
                words.append(parts[0])
                rows.append(np.asarray(parts[1:], dtype=np.float64))
        vecs = np.stack(rows)
    vecs = vecs / np.maximum(np.linalg.norm(vecs, axis=1, keepdims=True), 1e-12)
    return dict(zip(words, vecs))


def _topics(folder: str) -> List[List[str]]:
    with open(os.path.join(folder, "topics.json")) as f:
        return json.load(f)


def wmd_tables(path_models: str, path_save: str, vectors: Dict[str, np.ndarray],
               nr_tpcs_lst=(10, 20, 30, 40, 50), n_words_lst=(10, 50, 100, 200, 300),
               engine: Optional[str] = None):
    import pandas as pd
    if engine not in (None, "lp", "host", "device"):
        raise ValueError("engine must be None, 'lp', 'host' or 'device'")
    batched = engine in ("host", "device")
    names = sorted(n for n in os.listdir(path_models) if os.path.isdir(os.path.join(path_models, n)))
    centr = sorted((n for n in names if n.startswith("centralized")), key=lambda n: int(n.split("_")[1]))
    os.makedirs(path_save, exist_ok=True)
    written = []
    for k in nr_tpcs_lst:
        nodes = [n for n in names if n.startswith("non_collaborative") and int(n.split("_")[-3]) == k]
        if not nodes:
            continue
        cols = [f"Node {i + 1}" for i in range(len(nodes))] + [f"Centr {n.split('_')[1]}" for n in centr]
        every = nodes + centr
        for nw in n_words_lst:
            d = np.zeros((len(nodes), len(every)))
            vec = vectors
            if batched:                  # one table (one upload) of the words this table compares
                tops = {name: _topics(os.path.join(path_models, name)) for name in every}
                vec = WordTable(vectors, (w for ts in tops.values() for t in ts for w in t[:nw]),
                                device=engine == "device")
            for i, ref in enumerate(nodes):
                tr = _topics(os.path.join(path_models, ref))
                for j, cmp_ in enumerate(every):
                    d[i, j] = mean_min_wmd(tr, _topics(os.path.join(path_models, cmp_)), vec, nw,
                                           engine=engine)
            out = os.path.join(path_save, f"wmds_{k}tpcs_{nw}_words.csv")
            pd.DataFrame(d, index=cols[: len(nodes)], columns=cols).to_csv(out)
            written.append(out)
    return written


def main(argv=None):
    p = argparse.ArgumentParser(description="WMD between topic models")
    p.add_argument("--path_models", required=True)
    p.add_argument("--path_save", required=True)
    p.add_argument("--vectors", required=True, help="word2vec text file or .npz (words, vectors)")
    p.add_argument("--nr_tpcs_lst", type=str, default="10,20,30,40,50")
    p.add_argument("--n_words_lst", type=str, default="10,50,100,200,300")
    p.add_argument("--engine", default=None, choices=["lp", "host", "device"],
                   help="lp (default): one LP per topic pair; host / device: the batched exact "
                        "transport solver (numpy twin / HIP kernels)")
    a = p.parse_args(argv)
    return wmd_tables(a.path_models, a.path_save, load_vectors(a.vectors),
                      [int(x) for x in a.nr_tpcs_lst.split(",")],
                      [int(x) for x in a.n_words_lst.split(",")], engine=a.engine)


if __name__ == "__main__":
    main()
