"""Collapsed Gibbs sampling for LDA (csrc/gibbs.hip) and its numpy twin.

The sampler Mallet's ``ParallelTopicModel`` runs, with documents for threads: the
document-topic counts ``ndk`` are live, the word-topic counts ``nwk`` / ``nk`` are those at
the start of the sweep and are recounted from the assignments ``z`` after it.

Tokens: token ``i`` of document ``d`` counts in storage order of the CSR row, a non-zero
``(w, x)`` being ``x`` consecutive tokens.  Token ``i`` of global document ``g`` in sweep
``s`` (1, 2, ...; 0 is the initialisation) draws component ``i & 3`` of
``rng4(seed, step=s, tag=RNG_GIBBS | ((i >> 2) << 8), idx=g)`` through ``u01``:

  init    z = min(K - 1, floor(u K))                                         (fp32)
  sweep   ndk[o] -= 1;  p_k = (ndk[k] + alpha_k) (nwk0[w][k] - [k = o] + beta)
                               / (nk0[k] - [k = o] + V beta)                 (fp32)
          cum = inclusive prefix sum of p;  target = u cum[K - 1]
          k' = min(K - 1, #{k : cum_k <= target});  z = k';  ndk[k'] += 1

``frozen`` sweeps (fold-in of unseen documents against somebody else's counts) drop the
``[k = o]`` terms and never recount.

``engine``: ``"fused"`` (the kernels; raises off-GPU or without the kernel library),
``"host"`` (numpy: the CPU implementation, vectorised across documents by token position),
``None`` (fused for a :class:`DeviceCSR` on a GPU, host otherwise).  Within an engine a seed
names one trajectory, whatever the grid or the chunking.  The initial ``z`` is the same in
both engines; in a sweep the engines round ``cum`` differently (the kernel sums the lanes'
partial sums with a parallel prefix and divides with the hardware reciprocal), so a draw
that lands between the two values may pick the neighbouring topic, and the trajectories
part from there.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from ..data.bow import DeviceCSR, to_csr
from . import kernel_abi as abi
from . import native
from .thin import HOST_SLAB, MAX_COUNT, philox4x32_10

RNG_GIBBS = 7                # csrc/gfk_common.h
MAX_TOPICS = 512             # csrc/gibbs.hip LDA_MAX_K
MAX_DOC_TOKENS = 1 << 26     # the token block (i >> 2) << 8 stays in 32 bits
DOC_CHUNK = 1 << 20          # default documents per launch
SEG = 4096                   # non-zeros per recount work item (a frequent word is split)


def host_draws(seed: int, sweep: int, doc, pos) -> np.ndarray:
    """u [n] (fp32) of tokens ``pos`` of global documents ``doc`` in sweep ``sweep``."""
    seed = int(seed) % (1 << 64)
    doc, pos = np.asarray(doc, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    out = np.empty(len(doc), dtype=np.float32)
    for a in range(0, len(doc), HOST_SLAB):
        d, i = doc[a:a + HOST_SLAB], pos[a:a + HOST_SLAB]
        r = philox4x32_10(seed, d, int(sweep), RNG_GIBBS | ((i >> 2) << 8), 0x5EED)
        x = np.choose(i & 3, r)
        out[a:a + HOST_SLAB] = (x >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return out


def optimize_alpha(ndk: torch.Tensor, alpha, iters: int = 5) -> np.ndarray:
    """Minka's fixed point for an asymmetric Dirichlet prior on the document-topic counts:
    ``alpha_k <- alpha_k sum_d[psi(n_dk + alpha_k) - psi(alpha_k)] /
    sum_d[psi(n_d + sum alpha) - psi(sum alpha)]``, ``iters`` times, in float64 on the
    device of ``ndk``."""
    n = ndk.to(torch.float64)
    n = n[n.sum(1) > 0]
    a = torch.as_tensor(np.asarray(alpha, dtype=np.float64), device=n.device)
    if n.shape[0] == 0:
        return a.cpu().numpy().astype(np.float32)
    nd = n.sum(1)
    for _ in range(int(iters)):
        s = a.sum()
        num = (torch.digamma(n + a) - torch.digamma(a)).sum(0)
        den = (torch.digamma(nd + s) - torch.digamma(s)).sum()
        a = (a * num / den).clamp_min(1e-6)
    return a.cpu().numpy().astype(np.float32)


def _bad_counts():
    return ValueError(f"counts must be integers in 0..{MAX_COUNT} (and the CSR well formed)")


class GibbsSampler:
    """The state of one chain over one corpus: ``z`` [N] (int16 holding 0 .. K - 1),
    ``nwk`` [V, K], ``nk`` [K], ``ndk`` [D, K] (int32), as torch tensors on the corpus'
    device (fused) or on the CPU (host).  The constructor draws the initial assignments
    (sweep 0) and counts them.

    ``alpha``: [K] or a scalar alpha_k, >= 0 and not all zero (a topic with alpha_k = 0 and no
    token in a document has p_k = 0 there; ``cum_k <= target`` passes over it even when the
    draw is exactly 0); ``beta`` > 0.  ``counts=(nwk, nk)``: a frozen chain
    (fold-in): every sweep samples against these counts without own-token exclusion, and
    they are never rewritten.  ``doc0``: global index of the first document (RNG key).
    ``chunk`` / ``max_grid`` (fused): documents per launch / a cap on the workgroups;
    ``seg``: non-zeros per recount work item.  None of the three changes a result."""

    def __init__(self, data, n_topics: int, alpha, beta: float = 0.01, seed: int = 0,
                 engine: Optional[str] = None, counts=None, doc0: int = 0,
                 chunk: Optional[int] = None, max_grid: Optional[int] = None,
                 seg: Optional[int] = None):
        if engine not in (None, "fused", "host"):
            raise ValueError("engine must be None, 'fused' or 'host'")
        on_gpu = isinstance(data, DeviceCSR) and data.device.type == "cuda"
        if engine is None:
            engine = "fused" if on_gpu else "host"
        if engine == "fused":
            if isinstance(data, DeviceCSR) and not on_gpu:
                raise RuntimeError("engine='fused' needs the corpus on a GPU")
            if not torch.cuda.is_available():
                raise RuntimeError("engine='fused' needs a GPU")
        self.engine = engine
        self.K = int(n_topics)
        if not 1 <= self.K <= MAX_TOPICS:
            raise ValueError(f"n_topics must lie in 1..{MAX_TOPICS}")
        self.beta = float(np.float32(beta))
        if not self.beta > 0:
            raise ValueError("beta must be positive")
        self.seed, self.doc0 = int(seed) % (1 << 64), int(doc0)
        self.chunk = DOC_CHUNK if chunk is None else int(chunk)
        self.seg = SEG if seg is None else int(seg)
        if self.chunk < 1 or self.seg < 1 or self.doc0 < 0:
            raise ValueError("chunk and seg must be positive, doc0 non-negative")
        if max_grid is not None and int(max_grid) < 1:
            raise ValueError("max_grid must be a positive number of workgroups")
        self.max_grid = 0 if max_grid is None else int(max_grid)
        self.frozen = counts is not None
        self.sweeps = 0
        if engine == "fused":
            self._prepare_fused(data)
        else:
            self._prepare_host(data)
        self.vbeta = float(np.float32(self.V * np.float64(np.float32(self.beta))))
        self.set_alpha(alpha)
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        self.z = torch.zeros(max(self.N, 1), dtype=torch.int16, device=dev)
        self.ndk = torch.zeros(self.D, self.K, **i32)
        if self.frozen:
            nwk, nk = counts
            self.nwk = torch.as_tensor(nwk, device=dev).to(torch.int32).contiguous()
            self.nk = torch.as_tensor(nk, device=dev).to(torch.int32).contiguous()
            if tuple(self.nwk.shape) != (self.V, self.K) or tuple(self.nk.shape) != (self.K,):
                raise ValueError(f"counts must be nwk [{self.V}, {self.K}] and nk [{self.K}]")
        else:
            self.nwk = torch.zeros(self.V, self.K, **i32)
            self.nk = torch.zeros(self.K, **i32)
        self._init()

    # ------------------------------------------------------------------ corpus
    def _sizes(self, n_docs, V, N, doc_max):
        self.D, self.V, self.N = int(n_docs), int(V), int(N)
        if self.N >= 2**31:
            raise ValueError("the corpus must hold fewer than 2^31 tokens; split it")
        if doc_max > MAX_DOC_TOKENS:
            raise ValueError(f"a document may hold at most {MAX_DOC_TOKENS} tokens")
        if self.doc0 + self.D >= 2**31:
            raise ValueError("doc0 + documents must stay below 2^31")

    def _items(self, cnt: np.ndarray):
        """Recount work items from the words' non-zero counts: (lo, hi, row) per item and
        (word, first, n) per split word."""
        seg, V = self.seg, self.V
        nseg = np.maximum(1, (cnt + seg - 1) // seg)
        wp = np.cumsum(cnt) - cnt
        word = np.repeat(np.arange(V, dtype=np.int64), nseg)
        j = np.arange(len(word), dtype=np.int64) - np.repeat(np.cumsum(nseg) - nseg, nseg)
        lo = wp[word] + j * seg
        hi = np.minimum(lo + seg, wp[word] + cnt[word])
        split = nseg[word] > 1
        row = word.copy()
        row[split] = -1 - np.arange(int(split.sum()), dtype=np.int64)
        mw = np.flatnonzero(nseg > 1)
        mn = nseg[mw]
        return (lo, hi, row), (mw, np.cumsum(mn) - mn, mn), int(split.sum())

    def _prepare_host(self, data):
        if isinstance(data, DeviceCSR):
            indptr, indices = data.indptr.cpu().numpy(), data.indices.cpu().numpy()
            values, shape = data.values.cpu().numpy(), (data.n_docs, data.vocab_size)
        else:
            m = to_csr(data)
            indptr, indices, values, shape = m.indptr, m.indices, m.data, m.shape
        self.device = torch.device("cpu")
        if np.any((values != np.floor(values)) | (values < 0) | (values > MAX_COUNT)):
            raise _bad_counts()
        x = values.astype(np.int64)
        rows = np.repeat(np.arange(shape[0], dtype=np.int64), np.diff(indptr))
        lens = np.bincount(rows, weights=x, minlength=shape[0]).astype(np.int64)
        self._sizes(shape[0], shape[1], int(x.sum()), int(lens.max()) if len(lens) else 0)
        h = self._h = {}
        h["doc"] = np.repeat(rows, x)                                   # per token
        h["word"] = np.repeat(indices.astype(np.int64), x)
        h["pos"] = np.arange(self.N, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
        order = np.argsort(h["pos"], kind="stable")                     # tokens by position
        h["by_pos"] = np.split(order, np.cumsum(np.bincount(h["pos"]))[:-1]) if self.N else []

    def _prepare_fused(self, data):
        if not isinstance(data, DeviceCSR):
            data = DeviceCSR(data, "cuda")
        self.lib = native.kernels()
        if self.K > self.lib.gfk_lda_max_topics() or MAX_DOC_TOKENS != self.lib.gfk_lda_max_doc_tokens():
            raise RuntimeError("the kernel library's Gibbs limits differ from the launcher's")
        self.data, self.device = data, data.device
        dev = data.device
        V, nnz = int(data.vocab_size), int(data.indices.numel())
        v, ix, ip = data.values, data.indices, data.indptr
        i32 = dict(dtype=torch.int32, device=dev)
        self.tok_ptr = torch.zeros(nnz + 1, **i32)
        doc_max = total = 0
        if nnz:
            bad = ((v != v.floor()) | (v < 0) | (v > MAX_COUNT) | (ix < 0) | (ix >= V)).any() \
                | (ip[0] != 0) | (ip[-1] != nnz) | (ip[1:] < ip[:-1]).any()
            cum = torch.cumsum(v.to(torch.int64), 0)
            at = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), cum])[ip.long()]
            stats = torch.stack([bad.to(torch.int64), cum[-1], (at[1:] - at[:-1]).max()]).tolist()
            if stats[0]:                              # (the one sync of the checks)
                raise _bad_counts()
            total, doc_max = stats[1], stats[2]
        self._sizes(data.n_docs, V, total, doc_max)
        if nnz:
            self.tok_ptr[1:] = cum.to(torch.int32)
        # the inverted index: non-zeros by word, in storage order within a word
        self.inv = torch.sort(ix, stable=True).indices.to(torch.int32)
        cnt = torch.bincount(ix.long(), minlength=V).cpu().numpy().astype(np.int64) if nnz \
            else np.zeros(V, dtype=np.int64)
        items, merge, n_part = self._items(cnt)
        self.items = [torch.as_tensor(a, **i32) for a in items]
        self.merge = [torch.as_tensor(a, **i32) for a in merge]
        self.part = torch.empty(max(n_part, 1), self.K, **i32)

    def set_alpha(self, alpha) -> None:
        a = np.asarray(alpha, dtype=np.float32)
        a = np.full(self.K, a, dtype=np.float32) if a.ndim == 0 else a
        if a.shape != (self.K,) or not np.all(a >= 0) or not np.any(a > 0) \
                or not np.all(np.isfinite(a)):
            raise ValueError(f"alpha must hold {self.K} non-negative values, one of them positive")
        self.alpha = np.ascontiguousarray(a)
        self._alpha_t = torch.from_numpy(self.alpha).to(self.device)

    # ------------------------------------------------------------------ fused
    def _launch(self, pass_, sweep=0, store_ndk=True):
        if not self.N:                       # no token: the zeroed counts are already right
            return
        p = abi.GfkLda()
        p.tok_ptr, p.z = self.tok_ptr.data_ptr(), self.z.data_ptr()
        p.K, p.V, p.seed, p.max_grid, p.pass_ = self.K, self.V, self.seed, self.max_grid, pass_
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if pass_ in (abi.LDA_INIT, abi.LDA_SWEEP):
                p.indices = self.data.indices.data_ptr()
                p.nwk0, p.nk0 = self.nwk.data_ptr(), self.nk.data_ptr()
                p.alpha, p.beta, p.vbeta = self._alpha_t.data_ptr(), self.beta, self.vbeta
                p.sweep, p.frozen = int(sweep), int(self.frozen)
                for d0 in range(0, self.D, self.chunk):
                    p.indptr = self.data.indptr.data_ptr() + 4 * d0
                    p.n_docs, p.doc0 = min(self.D, d0 + self.chunk) - d0, self.doc0 + d0
                    p.ndk = self.ndk.data_ptr() + 4 * d0 * self.K if store_ndk else None
                    self._call(p, stream)
                return
            p.nwk, p.part = self.nwk.data_ptr(), self.part.data_ptr()
            if pass_ == abi.LDA_RECOUNT:
                p.inv = self.inv.data_ptr()
                p.item_lo, p.item_hi, p.item_row = (t.data_ptr() for t in self.items)
                p.n_items = int(self.items[0].numel())
            else:
                p.mrg_word, p.mrg_first, p.mrg_n = (t.data_ptr() for t in self.merge)
                p.n_items = int(self.merge[0].numel())
            self._call(p, stream)

    def _call(self, p, stream):
        rc = self.lib.gfk_lda(C.byref(p), stream)
        if rc:
            raise RuntimeError(f"gfk_lda failed ({rc})")

    def _recount_fused(self):
        self._launch(abi.LDA_RECOUNT)
        if self.merge[0].numel():
            self._launch(abi.LDA_MERGE)
        self.nk.copy_(self.nwk.sum(0, dtype=torch.int32))

    # ------------------------------------------------------------------ host
    def _recount_host(self):
        h, K = self._h, self.K
        z = self.z.numpy()[:self.N].astype(np.int64)
        nwk = np.bincount(h["word"] * K + z, minlength=self.V * K).reshape(self.V, K)
        self.nwk.copy_(torch.from_numpy(nwk.astype(np.int32)))
        self.nk.copy_(torch.from_numpy(nwk.sum(0).astype(np.int32)))

    def _ndk_host(self):
        z = self.z.numpy()[:self.N].astype(np.int64)
        return np.bincount(self._h["doc"] * self.K + z,
                           minlength=self.D * self.K).reshape(self.D, self.K).astype(np.int32)

    def _sweep_host(self, sweep, _variant=()):
        """One sweep of the twin.  ``_variant``: deliberately wrong samplers, for the tests
        that pin the sweep oracle ("no_exclusion", "alpha_shift", "strict", "no_decrement",
        "live_nk")."""
        h, K = self._h, self.K
        z = self.z.numpy()
        nd = self._ndk_host()
        nwk0, nk0 = self.nwk.numpy(), self.nk.numpy().copy()
        alpha = np.roll(self.alpha, 1) if "alpha_shift" in _variant else self.alpha
        beta, vbeta = np.float32(self.beta), np.float32(self.vbeta)
        exclude = not self.frozen and "no_exclusion" not in _variant
        u_all = host_draws(self.seed, sweep, self.doc0 + h["doc"], h["pos"])
        for idx in h["by_pos"]:
            d, w, o = h["doc"][idx], h["word"][idx], z[idx].astype(np.int64)
            r = np.arange(len(idx))
            if "no_decrement" not in _variant:
                nd[d, o] -= 1
            nw = nwk0[w]
            nk = np.broadcast_to(nk0, nw.shape)
            if exclude:
                nw, nk = nw.copy(), nk.copy()
                nw[r, o] -= 1
                nk[r, o] -= 1
            p = (nd[d].astype(np.float32) + alpha) * (nw.astype(np.float32) + beta) \
                / (nk.astype(np.float32) + vbeta)
            cum = np.cumsum(p, axis=1, dtype=np.float32)
            target = u_all[idx] * cum[:, -1]
            hit = cum < target[:, None] if "strict" in _variant else cum <= target[:, None]
            k = np.minimum(K - 1, hit.sum(1))
            z[idx] = k.astype(np.int16)
            if "no_decrement" in _variant:
                nd[d, o] -= 1
            nd[d, k] += 1
            if "live_nk" in _variant:
                np.subtract.at(nk0, o, 1)
                np.add.at(nk0, k, 1)
        self.ndk.copy_(torch.from_numpy(nd))

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def _init(self):
        if self.engine == "fused":
            self._launch(abi.LDA_INIT)
        elif self.N:
            h = self._h
            u = host_draws(self.seed, 0, self.doc0 + h["doc"], h["pos"])
            k = np.floor(u * np.float32(self.K)).astype(np.int64)
            self.z.numpy()[:self.N] = np.minimum(self.K - 1, k).astype(np.int16)
        self.recount(ndk=True)

    @torch.no_grad()
    def recount(self, ndk: bool = False):
        """``nwk`` / ``nk`` from ``z`` (not on a frozen chain); ``ndk`` too when asked."""
        if not self.frozen:
            self._recount_fused() if self.engine == "fused" else self._recount_host()
        if ndk:
            if self.engine == "host":
                self.ndk.copy_(torch.from_numpy(self._ndk_host()))
            else:
                doc = torch.repeat_interleave(
                    torch.arange(self.D, device=self.device),
                    (self.tok_ptr[self.data.indptr[1:].long()]
                     - self.tok_ptr[self.data.indptr[:-1].long()]).long())
                flat = torch.bincount(doc * self.K + self.z[:self.N].long(),
                                      minlength=self.D * self.K)
                self.ndk.copy_(flat.view(self.D, self.K).to(torch.int32))

    @torch.no_grad()
    def sweep(self, n: int = 1, _variant=()):
        """``n`` sweeps: every token resampled in order, then (not frozen) the recount.
        ``ndk`` holds the counts the last sweep left."""
        for _ in range(int(n)):
            self.sweeps += 1
            if self.engine == "fused":
                if _variant:
                    raise ValueError("the variants belong to the host engine")
                self._launch(abi.LDA_SWEEP, self.sweeps)
            else:
                self._sweep_host(self.sweeps, _variant)
            self.recount()
        return self
