"""Topic-model quality metrics.

* TSS / DSS on synthetic ground truth -- reference experiments/dss_tss/run_simulation.py:321-355
  and federated_avitm.py:152-193.  numpy on the host by default; ``engine="device"`` (and
  CUDA tensor inputs) take both in float64 on the matrix cores from 64 x 64 tiles, with no
  [D, D] matrix (csrc/simscore.hip, ops/simscore.py).
* NPMI coherence -- the reference delegates to the (missing) topicmodeler/gensim
  ``c_npmi`` (tm_wrapper.py:358-384).  Defined here precisely: for the top-N
  words of each topic, the mean over unordered word pairs of
  log((P(wi,wj)+eps) / (P(wi) P(wj))) / -log(P(wi,wj)+eps), eps = 1e-12, with
  probabilities estimated from document co-occurrence in a reference corpus
  (bag-of-words data has no word order, so there is no sliding window).  The
  co-occurrence counts are one GEMM on the device: D_bin[:, W]^T D_bin[:, W]
  over the union W of all topics' top words (``npmi_coherence``).  The counts are
  integers, so they can also be taken exactly where the documents are -- on a device CSR
  (csrc/cooc.hip) or a host CSR, per client -- and summed: ``cooccurrence_counts``,
  ``federated_cooccurrence``, ``npmi_from_counts`` (the same float64 formula).
* Topic diversity (TD) and rank-biased overlap (RBO) -- tm_wrapper.py:386-400.
* Word-mover's distance between topic sets given word vectors -- aux_scripts/evaluation/wmd.py:
  one LP per topic pair by default; ``engine="host"`` / ``"device"`` solve the whole
  [K_ref, K_cmp] batch with the exact transport solver of ops/wmd.py (csrc/wmd.hip).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import scipy.sparse as sp
import torch


def _sim_engine(engine: Optional[str], *operands) -> str:
    """"host" or "device" for the similarity scores: None follows the operands (CUDA tensors
    -> the kernels of csrc/simscore.hip, anything else -> numpy)."""
    if engine not in (None, "host", "device"):
        raise ValueError("engine must be None, 'host' or 'device'")
    if engine is None:
        engine = "device" if any(torch.is_tensor(o) and o.is_cuda for o in operands) else "host"
    if engine == "device" and not torch.cuda.is_available():
        raise RuntimeError("engine='device' needs a GPU")
    return engine


def _sim_operands(engine: str, *operands):
    """The operands as numpy arrays (host) or fp32 / fp64 CUDA tensors (device: numpy inputs
    are uploaded, onto the device of the first CUDA operand if there is one)."""
    operands = [o if torch.is_tensor(o) else np.asarray(o) for o in operands]
    for o in operands:
        if len(o.shape) != 2:
            raise ValueError(f"expected 2-D operands, got shape {tuple(o.shape)}")
    if engine == "host":
        return [o.detach().cpu().numpy() if torch.is_tensor(o) else o for o in operands]
    dev = next((o.device for o in operands if torch.is_tensor(o) and o.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    out = []
    for o in operands:
        t = o.detach() if torch.is_tensor(o) else torch.tensor(o)
        if t.dtype not in (torch.float32, torch.float64):
            t = t.double()
        out.append(t.to(dev))
    return out


def bhattacharyya(x, y, engine: Optional[str] = None):
    """Bhattacharyya coefficients ``BC[i][j] = sum_l sqrt(x[i][l] y[j][l])`` of the rows of
    ``x`` [M, L] and ``y`` [N, L] in float64: a numpy array on the host, a tensor on the
    operands' device from the kernels (``engine`` as for :func:`tss`)."""
    engine = _sim_engine(engine, x, y)
    x, y = _sim_operands(engine, x, y)
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"rows of {x.shape[1]} and {y.shape[1]} entries cannot be compared")
    if engine == "device":
        from ..ops import simscore
        return simscore.bhattacharyya(x, y)
    return np.sqrt(np.asarray(x, dtype=np.float64)).dot(np.sqrt(np.asarray(y, dtype=np.float64)).T)


def tss(betas, topic_vectors, engine: Optional[str] = None) -> float:
    """Topic similarity score: sum over ground-truth topics of the best Bhattacharyya
    coefficient with a learned topic (run_simulation.py:321-334).

    ``engine``: "host" -- the numpy product, in the dtype of the inputs; "device" -- the
    float64 matrix-core kernels of csrc/simscore.hip whatever the inputs' dtype (numpy inputs
    are uploaded; raises without a GPU or the kernel library); None -- device for CUDA
    tensors, host otherwise."""
    engine = _sim_engine(engine, betas, topic_vectors)
    betas, topic_vectors = _sim_operands(engine, betas, topic_vectors)
    if betas.shape[1] != topic_vectors.shape[1]:
        raise ValueError(f"topics over {betas.shape[1]} and {topic_vectors.shape[1]} words "
                         "cannot be compared")
    if engine == "device":
        from ..ops import simscore
        return float(simscore.tss(betas, topic_vectors).item())
    return float(np.sum(np.max(np.sqrt(betas).dot(np.sqrt(topic_vectors.T)), axis=0)))


def dss(thetas_true, thetas, n_docs: Optional[int] = None, engine: Optional[str] = None) -> float:
    """Document similarity score (run_simulation.py:337-355).  ``engine`` as for :func:`tss`;
    the host formula builds two dense [D, D] matrices, the device path 64 x 64 tiles of them."""
    engine = _sim_engine(engine, thetas_true, thetas)
    thetas_true, thetas = _sim_operands(engine, thetas_true, thetas)
    if thetas_true.shape[0] != thetas.shape[0]:
        raise ValueError(f"thetas_true has {thetas_true.shape[0]} documents, thetas "
                         f"{thetas.shape[0]}")
    n_docs = len(thetas_true) if n_docs is None else n_docs
    if engine == "device":
        from ..ops import simscore
        return float(simscore.dss(thetas_true, thetas, n_docs).item())
    a = np.sqrt(thetas_true).dot(np.sqrt(thetas_true.T))
    b = np.sqrt(thetas).dot(np.sqrt(thetas.T))
    return float(np.sum(np.abs(a - b)) / n_docs)


def betas_to_ground_truth_vocab(betas: np.ndarray, id2token: Dict[int, str], vocab_size: int,
                                prefix: str = "wd") -> np.ndarray:
    """Re-index a [K, V_learned] topic-word matrix onto the generator vocabulary
    ('wd<j>' -> column j), zero elsewhere, L1-normalised (reference
    auxiliary_functions.py:441-483, vectorised)."""
    out = np.zeros((betas.shape[0], vocab_size), dtype=np.float64)
    cols = np.array([int(id2token[i][len(prefix):]) for i in range(betas.shape[1])])
    out[:, cols] = betas
    s = out.sum(axis=1, keepdims=True)
    s[s == 0] = 1.0
    return out / s


def npmi_coherence(topics: Sequence[Sequence[int]], corpus: sp.csr_matrix, eps: float = 1e-12,
                   per_topic: bool = False, device=None):
    """NPMI of topics given as vocabulary indices, on a reference doc-term matrix."""
    topics = [list(map(int, t)) for t in topics]
    words = sorted({w for t in topics for w in t})
    pos = {w: i for i, w in enumerate(words)}
    sub = (corpus[:, words] > 0).astype(np.float32)
    n_docs = corpus.shape[0]
    dev = torch.device(device) if device is not None else torch.device("cpu")
    d = torch.from_numpy(sub.toarray()).to(dev)
    co = (d.t() @ d).double() / n_docs          # P(wi, wj); diagonal = P(wi)
    scores = _npmi_scores(topics, pos, co, eps, dev)
    return scores if per_topic else float(np.mean(scores))


def _npmi_scores(topics, pos, co, eps, dev) -> List[float]:
    """Per-topic NPMI from the float64 joint probabilities ``co`` [W, W] (diagonal = P(wi));
    ``pos`` maps a word to its row.  The one body behind :func:`npmi_coherence` and
    :func:`npmi_from_counts`."""
    p = torch.diagonal(co)
    scores = []
    for t in topics:
        idx = torch.tensor([pos[w] for w in t], device=dev)
        pij = co[idx][:, idx]
        pi = p[idx]
        pmi = torch.log((pij + eps) / (pi[:, None] * pi[None, :] + 1e-300))
        npmi = pmi / (-torch.log(pij + eps))
        iu = torch.triu_indices(len(t), len(t), 1, device=dev)
        scores.append(float(npmi[iu[0], iu[1]].mean().item()))
    return scores


def npmi_from_counts(topics: Sequence[Sequence[int]], words: Sequence[int], counts, n_docs: int,
                     eps: float = 1e-12, per_topic: bool = False):
    """:func:`npmi_coherence` from exact integer document co-occurrence counts:
    ``counts[i][j]`` = documents holding both ``words[i]`` and ``words[j]`` (the diagonal is
    the document frequency), out of ``n_docs``.  The same float64 formula, on the CPU; with
    the counts of the same corpus the result is bit-identical to :func:`npmi_coherence`."""
    topics = [list(map(int, t)) for t in topics]
    if torch.is_tensor(words):
        words = words.detach().cpu().tolist()
    pos = {int(w): i for i, w in enumerate(words)}
    dev = torch.device("cpu")
    c = counts.detach().to(dev) if torch.is_tensor(counts) else torch.from_numpy(np.asarray(counts))
    co = c.double() / n_docs
    scores = _npmi_scores(topics, pos, co, eps, dev)
    return scores if per_topic else float(np.mean(scores))


def _word_tensor(words, vocab_size: int) -> torch.Tensor:
    """``words`` as an int64 tensor (kept on its device when it is one); distinct indices in
    [0, vocab_size) or ValueError."""
    if torch.is_tensor(words):
        w = words.detach().reshape(-1)
        if w.dtype.is_floating_point or w.dtype == torch.bool:
            raise ValueError("words must be integer vocabulary indices")
        w = w.long()
    else:
        w = torch.from_numpy(np.asarray(list(words), dtype=np.int64).reshape(-1))
    if w.numel():
        if int(w.min()) < 0 or int(w.max()) >= vocab_size:
            raise ValueError(f"words must be vocabulary indices in [0, {vocab_size})")
        if int(torch.unique(w).numel()) != int(w.numel()):
            raise ValueError("words must be distinct")
    return w


def _host_csr(data) -> sp.csr_matrix:
    if sp.issparse(data):
        return sp.csr_matrix(data)
    return sp.csr_matrix((data.values.cpu().numpy(), data.indices.cpu().numpy(),
                          data.indptr.cpu().numpy()), shape=(data.n_docs, data.vocab_size))


def _cooccurrence(data, words, engine: Optional[str], chunk: Optional[int],
                  max_grid: Optional[int] = None):
    """(counts, engine used) -- :func:`cooccurrence_counts` plus which implementation ran."""
    from ..data.bow import DeviceCSR
    from ..ops import cooc
    if engine not in (None, "fused", "exact"):
        raise ValueError("engine must be None, 'fused' or 'exact'")
    if not (isinstance(data, DeviceCSR) or sp.issparse(data)):
        raise TypeError("data must be a DeviceCSR or a scipy sparse matrix")
    on_device = isinstance(data, DeviceCSR)
    vocab_size = int(data.vocab_size if on_device else data.shape[1])
    w = _word_tensor(words, vocab_size)
    device = data.device if on_device else torch.device("cpu")
    if engine == "fused":
        if not on_device:
            if not torch.cuda.is_available():
                raise RuntimeError("engine='fused' needs a GPU")
            data = DeviceCSR(data, torch.device("cuda", torch.cuda.current_device()))
            device = data.device
        elif device.type != "cuda":
            raise RuntimeError("engine='fused' needs the data on a GPU")
    elif engine is None and on_device and device.type == "cuda":
        # on a GPU the kernels are the path: a missing library raises, only a word list past
        # their limit goes to the host (and says so)
        if int(w.numel()) <= cooc.max_words():
            engine = "fused"
        else:
            import logging
            logging.getLogger("gfedntm_amd").info(
                "co-occurrence counts: %d words exceed the kernels' %d, using the host product",
                int(w.numel()), cooc.max_words())
    if engine == "fused":
        return cooc.counts(data, w.to(device), chunk, max_grid), "fused"
    if chunk is not None and int(chunk) < 1:
        raise ValueError("chunk must be a positive number of documents")
    xb = (_host_csr(data)[:, w.cpu().numpy()] > 0).astype(np.int64)
    co = np.asarray((xb.T @ xb).todense(), dtype=np.int64).reshape(len(w), len(w))
    return torch.from_numpy(co).to(device), "exact"


def cooccurrence_counts(data, words: Sequence[int], engine: Optional[str] = None,
                        chunk: Optional[int] = None, max_grid: Optional[int] = None) -> torch.Tensor:
    """Exact document co-occurrence counts of ``words`` in ``data``: int64 [W, W] on the
    data's device, ``[i][j]`` = documents in which ``words[i]`` and ``words[j]`` both have a
    stored value > 0 (diagonal: document frequency).

    ``data``: a :class:`~gfedntm_amd.data.bow.DeviceCSR` or a scipy sparse matrix; ``words``:
    distinct vocabulary indices in any order.  ``engine``: "fused" -- the bit-matrix kernels
    of csrc/cooc.hip on the device CSR (raises off-GPU, without the kernel library, or past
    the kernels' word limit); "exact" -- the sparse integer product Xb^T Xb on the host
    (scipy; no dense [D, W] either); None -- fused for a DeviceCSR on a GPU within the
    limit, exact otherwise.  ``chunk``: documents per launch of the fused path (any positive
    number; by default the bit matrix stays at or below 256 MiB).  The counts are integers:
    neither engine, chunking nor grid changes them (``max_grid`` caps the fused pack kernel's
    workgroups: ops/cooc.py)."""
    return _cooccurrence(data, words, engine, chunk, max_grid)[0]


def _federated_cooccurrence(datas, words, group=None, engine: Optional[str] = None):
    datas = list(datas)
    counts, n_docs, engines = None, 0, []
    for d in datas:
        c, e = _cooccurrence(d, words, engine, None)
        counts = c if counts is None else counts + c.to(counts.device)
        n_docs += int(d.n_docs if hasattr(d, "n_docs") else d.shape[0])
        engines.append(e)
    if counts is None:
        nw = int(words.numel()) if torch.is_tensor(words) else len(list(words))
        counts = torch.zeros(nw, nw, dtype=torch.int64)
    import torch.distributed as dist
    if group is not False and (group is not None or (dist.is_available() and dist.is_initialized())):
        shape, dev = counts.shape, counts.device
        buf = torch.cat([counts.reshape(-1), torch.tensor([n_docs], dtype=torch.int64, device=dev)])
        # gloo reduces host tensors, RCCL device tensors: stage the (small) buffer where the
        # group's backend wants it
        backend = str(dist.get_backend(group))
        if backend == "gloo" and buf.is_cuda:
            buf = buf.cpu()
        elif backend == "nccl" and not buf.is_cuda:
            buf = buf.cuda()
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        buf = buf.to(dev)
        counts, n_docs = buf[:-1].reshape(shape), int(buf[-1])
    used = "fused" if engines and all(e == "fused" for e in engines) else "exact"
    return counts, n_docs, used


def federated_cooccurrence(datas, words: Sequence[int], group=None):
    """(counts int64 [W, W], n_docs) of the union of document shards that stay where they
    are: :func:`cooccurrence_counts` of each of this process's ``datas`` summed, then -- when
    ``group`` is a process group, or a default group is initialised and ``group`` is not
    False -- one ``all_reduce(SUM)`` of the matrix and the document count over the ranks.
    Integer sums do not depend on their order, so the result equals the counts of the
    stacked corpus exactly; only W^2 + 1 integers leave a process.  ``words`` must be the
    same list on every rank."""
    counts, n_docs, _ = _federated_cooccurrence(datas, words, group)
    return counts, n_docs


def topic_diversity(topics: Sequence[Sequence], topk: int = 25) -> float:
    """Fraction of unique words among the top-k words of all topics."""
    words = [w for t in topics for w in list(t)[:topk]]
    return len(set(words)) / max(len(words), 1)


def rbo(list1: Sequence, list2: Sequence, p: float = 0.9) -> float:
    """Extrapolated rank-biased overlap of two ranked lists (Webber et al. 2010)."""
    k = max(len(list1), len(list2))
    if k == 0:
        return 1.0
    x = 0
    s1, s2 = set(), set()
    summ = 0.0
    for d in range(1, k + 1):
        a = list1[d - 1] if d <= len(list1) else None
        b = list2[d - 1] if d <= len(list2) else None
        if a == b and a is not None:
            x += 1
        else:
            if a is not None and a in s2:
                x += 1
            if b is not None and b in s1:
                x += 1
        if a is not None:
            s1.add(a)
        if b is not None:
            s2.add(b)
        summ += (x / d) * p ** d
    return float((x / k) * p ** k + (1 - p) / p * summ)


def inverted_rbo(topics: Sequence[Sequence], topk: int = 10, p: float = 0.9) -> float:
    """1 - mean pairwise RBO between topics (topic distinctness)."""
    n = len(topics)
    if n < 2:
        return 1.0
    vals = [rbo(list(topics[i])[:topk], list(topics[j])[:topk], p)
            for i in range(n) for j in range(i + 1, n)]
    return float(1.0 - np.mean(vals))


_WMD_ENGINES = (None, "lp", "host", "device")


class WordTable:
    """Word vectors as one [W, dim] float64 table plus ``index`` (word -> row), for the batched
    WMD engines: built once (``device=True``: uploaded once) and shared by every
    :func:`mean_min_wmd` call that compares topics over these words.  Reads like the dict it
    was built from (``word in table``, ``table[word]``)."""

    def __init__(self, vectors: Dict[str, np.ndarray], words=None, device: bool = False):
        keep = list(vectors) if words is None else [w for w in dict.fromkeys(words) if w in vectors]
        self.index = {w: i for i, w in enumerate(keep)}
        self.host = (np.stack([np.asarray(vectors[w], dtype=np.float64) for w in keep])
                     if keep else np.zeros((0, 0)))
        self.table = self.host
        if device:
            import torch
            self.table = torch.from_numpy(self.host).cuda()

    def __contains__(self, word) -> bool:
        return word in self.index

    def __getitem__(self, word) -> np.ndarray:
        return self.host[self.index[word]]


def _wmd_batched(lists1, lists2, vectors, engine) -> np.ndarray:
    """[len(lists1), len(lists2)] WMDs of word lists on the "host" / "device" engine
    (ops/wmd.py); words without a vector are dropped, a list left empty gives inf."""
    from ..ops import wmd
    if not isinstance(vectors, WordTable):
        vectors = WordTable(vectors, (w for l in list(lists1) + list(lists2) for w in l))
    ix = vectors.index
    la = [[ix[w] for w in l if w in ix] for l in lists1]
    lb = [[ix[w] for w in l if w in ix] for l in lists2]
    if not ix:
        return np.full((len(la), len(lb)), np.inf)
    return wmd.pairwise_wmd(la, lb, vectors.table, engine=engine)


def word_movers_distance(words1: Sequence[str], words2: Sequence[str], vectors: Dict[str, np.ndarray],
                         engine: Optional[str] = None) -> float:
    """WMD between two bags of words with uniform weights.  ``engine``: None / "lp" -- exact EMD
    via one LP (scipy HiGHS); "host" / "device" -- the exact transport solver of ops/wmd.py
    (numpy twin / csrc/wmd.hip kernels)."""
    if engine not in _WMD_ENGINES:
        raise ValueError("engine must be None, 'lp', 'host' or 'device'")
    if engine in ("host", "device"):
        return float(_wmd_batched([list(words1)], [list(words2)], vectors, engine)[0, 0])
    from scipy.optimize import linprog
    a = [w for w in words1 if w in vectors]
    b = [w for w in words2 if w in vectors]
    if not a or not b:
        return float("inf")
    va = np.stack([vectors[w] for w in a])
    vb = np.stack([vectors[w] for w in b])
    cost = np.sqrt(((va[:, None, :] - vb[None, :, :]) ** 2).sum(-1))
    n, m = cost.shape
    A_eq, b_eq = [], []
    for i in range(n):
        row = np.zeros(n * m); row[i * m:(i + 1) * m] = 1; A_eq.append(row); b_eq.append(1.0 / n)
    for j in range(m):
        row = np.zeros(n * m); row[j::m] = 1; A_eq.append(row); b_eq.append(1.0 / m)
    res = linprog(cost.ravel(), A_eq=np.array(A_eq), b_eq=np.array(b_eq), bounds=(0, None),
                  method="highs")
    return float(res.fun)


def mean_min_wmd(topics_ref: List[List[str]], topics_cmp: List[List[str]],
                 vectors: Dict[str, np.ndarray], n_words: int = 10,
                 engine: Optional[str] = None) -> float:
    """Mean over reference topics of the minimum WMD to any compared topic (wmd.py:56-80).
    ``engine`` as in :func:`word_movers_distance`; "host" / "device" take the whole
    [K_ref, K_cmp] matrix in one batched call (``vectors`` may be a :class:`WordTable`)."""
    if engine not in _WMD_ENGINES:
        raise ValueError("engine must be None, 'lp', 'host' or 'device'")
    if engine in ("host", "device"):
        d = _wmd_batched([t[:n_words] for t in topics_ref], [t[:n_words] for t in topics_cmp],
                         vectors, engine)
    else:
        d = np.array([[word_movers_distance(t1[:n_words], t2[:n_words], vectors) for t2 in topics_cmp]
                      for t1 in topics_ref])
    return float(np.mean(np.min(d, axis=1)))
