"""Gibbs-sampled LDA: the classical baseline the reference trains with Mallet
(``ParallelTopicModel``), here on the sampler of :mod:`gfedntm_amd.ops.lda`.

Hyperparameters keep Mallet's meaning: ``alpha`` is the SUM over topics (alpha_k = alpha /
K), ``beta`` the per-word smoothing, ``optimize_interval`` > 0 re-estimates an asymmetric
alpha every that many sweeps once ``burn_in`` sweeps have run (0: alpha stays symmetric).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..data.bow import DeviceCSR
from ..ops import lda


class GibbsLDA:
    def __init__(self, n_components: int = 10, alpha: float = 5.0, beta: float = 0.01,
                 num_iterations: int = 1000, optimize_interval: int = 10, burn_in: int = 200,
                 fold_in_burn_in: int = 20, seed: int = 0, device=None,
                 engine: Optional[str] = None):
        if n_components < 1 or not alpha > 0 or not beta > 0:
            raise ValueError("n_components, alpha and beta must be positive")
        self.n_components = int(n_components)
        self.alpha_sum, self.beta = float(alpha), float(beta)
        self.num_iterations = int(num_iterations)
        self.optimize_interval, self.burn_in = int(optimize_interval), int(burn_in)
        self.fold_in_burn_in = int(fold_in_burn_in)
        self.seed = int(seed)
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        if engine not in (None, "fused", "host"):
            raise ValueError("engine must be None, 'fused' or 'host'")
        self.engine = engine or ("fused" if self.device.type == "cuda" else "host")
        self.alphas = np.full(self.n_components, self.alpha_sum / self.n_components, np.float32)
        self.sampler = None
        self.train_data = None
        self.idx2token = None

    # ------------------------------------------------------------------ data
    def _corpus(self, dataset):
        """What the sampler takes: a DeviceCSR on the model's GPU (fused), else a scipy CSR."""
        if isinstance(dataset, DeviceCSR):
            return dataset
        csr = dataset.csr if hasattr(dataset, "csr") else dataset
        return DeviceCSR(csr, self.device) if self.engine == "fused" else csr

    def engine_info(self) -> dict:
        return {"engine": self.engine, "sampler": "csrc/gibbs.hip" if self.engine == "fused"
                else "numpy twin (ops/lda.py)"}

    # ------------------------------------------------------------------ training
    def fit(self, dataset, n_samples: Optional[int] = None):
        """``num_iterations`` sweeps over ``dataset`` (a BOWDataset / CTMDataset, a matrix or
        a DeviceCSR).  ``n_samples`` is accepted for the neural models' signature."""
        self.idx2token = getattr(dataset, "idx2token", None)
        self.train_data = dataset
        s = self.sampler = lda.GibbsSampler(self._corpus(dataset), self.n_components, self.alphas,
                                            self.beta, self.seed, engine=self.engine)
        for it in range(1, self.num_iterations + 1):
            s.sweep()
            if self.optimize_interval > 0 and it >= self.burn_in and it % self.optimize_interval == 0 \
                    and it < self.num_iterations:
                self.alphas = lda.optimize_alpha(s.ndk, s.alpha)
                s.set_alpha(self.alphas)
        if self.num_iterations == 0:
            s.recount(ndk=True)
        return self

    def _fitted(self):
        if self.sampler is None:
            raise RuntimeError("fit the model first")
        return self.sampler

    # ------------------------------------------------------------------ distributions
    def get_topic_word_distribution(self) -> np.ndarray:
        """[K, V]: (nwk + beta) / (nk + V beta)."""
        s = self._fitted()
        nwk, nk = s.nwk.double(), s.nk.double()
        return ((nwk + s.beta) / (nk + s.V * s.beta)).t().contiguous().cpu().numpy()

    def _theta(self, ndk: torch.Tensor) -> np.ndarray:
        a = torch.as_tensor(self.alphas.astype(np.float64), device=ndk.device)
        n = ndk.double() + a
        return (n / n.sum(1, keepdim=True)).cpu().numpy()

    def get_doc_topic_distribution(self, dataset, n_samples: int = 20) -> np.ndarray:
        """[D, K].  The training set: (ndk + alpha) / (n_d + sum alpha) of the chain.  Any
        other corpus is folded in: a frozen chain against the trained counts,
        ``fold_in_burn_in`` sweeps, then the mean of ``n_samples`` sweeps' ndk."""
        s = self._fitted()
        if dataset is self.train_data:
            return self._theta(s.ndk)
        f = lda.GibbsSampler(self._corpus(dataset), self.n_components, self.alphas, self.beta,
                             self.seed + 1, engine=self.engine, counts=(s.nwk, s.nk))
        f.sweep(self.fold_in_burn_in)
        acc = torch.zeros_like(f.ndk, dtype=torch.float64)
        n_samples = max(1, int(n_samples))
        for _ in range(n_samples):
            f.sweep()
            acc += f.ndk
        return self._theta(acc / n_samples)

    def get_topics(self, k: int = 10):
        s = self._fitted()
        if k > s.V:
            raise ValueError("k must be <= input size")
        top = torch.topk(s.nwk.t().double(), k, dim=1).indices.cpu().numpy()
        tok = self.idx2token or {i: str(i) for i in range(s.V)}
        return [[tok[int(i)] for i in row] for row in top]
