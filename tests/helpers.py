"""Shared fixtures for tests: tiny synthetic corpora."""
import numpy as np
import scipy.sparse as sp

from gfedntm_amd.data.synthetic import generate_synthetic, node_vocabulary_terms, remap_to_vocabulary
from gfedntm_amd.data.vocab import union_vocabulary, vocabulary_dict


def tiny_corpus(V=300, K=8, n_docs=100, n_nodes=2, seed=0, nwords=(30, 60)):
    c = generate_synthetic(vocab_size=V, n_topics=K, n_docs=n_docs, n_nodes=n_nodes,
                           frozen_topics=2, seed=seed, nwords=nwords)
    terms = union_vocabulary([node_vocabulary_terms(c, i) for i in range(n_nodes)])
    voc = vocabulary_dict(terms)
    shards = [remap_to_vocabulary(c, i, voc) for i in range(n_nodes)]
    return c, terms, shards


def random_csr(n_docs, V, nnz_per_row, seed=0):
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for d in range(n_docs):
        k = rng.integers(1, nnz_per_row + 1)
        c = rng.choice(V, size=min(k, V), replace=False)
        rows += [d] * len(c)
        cols += list(c)
        vals += list(rng.integers(1, 5, size=len(c)).astype(np.float32))
    m = sp.csr_matrix((vals, (rows, cols)), shape=(n_docs, V), dtype=np.float32)
    m.sort_indices()
    return m


def edge_csr(n_docs, V, nnz_per_row, plan, s_partial, seed=0, tile=64):
    """``random_csr`` with the rows a kernel can go wrong on, placed by the batch plan (so
    no seed search): returns (csr, {edge name: document id}).

    * ``empty_standin``: document ``plan.batch(s_partial)[0]`` is empty -- row 0 of the short
      batch, the document every dead row of that batch repeats;
    * ``empty_first`` / ``empty_last``: document ids 0 and n_docs - 1 are empty;
    * ``col0`` / ``col_last``: a single non-zero at column 0 / V - 1;
    * ``last_tile``: all non-zeros in the last (partial, if V % tile) ``tile``-word tile;
    * ``count1000``: one count of 1000;
    * ``every_tile``: one non-zero in every tile.
    The five non-empty ones are the first documents of the plan's first epoch that are
    not among the empty ones."""
    rng = np.random.default_rng(seed + 1)
    x = random_csr(n_docs, V, nnz_per_row, seed=seed).toarray()
    marks = {"empty_standin": int(plan.batch(s_partial)[0]), "empty_first": 0,
             "empty_last": n_docs - 1}
    for d in marks.values():
        x[d] = 0
    free = [int(d) for d in plan.order[:n_docs] if int(d) not in marks.values()]
    n_tiles = -(-V // tile)
    last0 = (n_tiles - 1) * tile
    for name, d in zip(("col0", "col_last", "last_tile", "count1000", "every_tile"), free):
        marks[name] = d
        if name == "count1000":
            x[d, np.flatnonzero(x[d])[0]] = 1000
            continue
        x[d] = 0
        if name == "col0":
            x[d, 0] = 2
        elif name == "col_last":
            x[d, V - 1] = 3
        elif name == "last_tile":
            cols = rng.choice(np.arange(last0, V), size=min(5, V - last0), replace=False)
            x[d, cols] = rng.integers(1, 5, size=len(cols))
        else:
            for t in range(n_tiles):
                x[d, rng.integers(t * tile, min((t + 1) * tile, V))] = rng.integers(1, 5)
    m = sp.csr_matrix(x, dtype=np.float32)
    m.sort_indices()
    return m, marks
